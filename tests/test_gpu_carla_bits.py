"""The CaRL agent's results, bit for bit, against a recording of the commit before the network table and
the split of ppo_carla.hip (tests/golden/carla_bits_parent/bits.npz, recorded on an MI355X from a build of
that parent commit). The CaRL kernels sum in fixed orders with no atomics, so the same launches give the
same bits: there are no tolerances here.

Cases (seed 7, 192 x 192 bev, inputs of carla_inputs, parameters of carla_ln_ref.init_params, which are
carla_inputs.params for an arch without LayerNorm; env_base 3, step_id 5):
  default arch, max_batch 65: forward at n = 7 in the four sample types (staged tail with the pre_lin path,
  ragged 16-row tiles) and at n = 65 given / sample (per-layer path with its split-K finish, k_carla_pack and
  k_carla_head, one row past the fused tail's limit); two consecutive updates at n = 7 and at n = 65 (the
  backward over both forward paths; the second step reads the Adam state), hyper-parameters and targets of
  test_gpu_carla.test_staged_conv1_kernels_match_generic.
  archs mlp, enc, full_nopol, full of test_gpu_carla_ln_agent.ARCHS, n = 4, max_batch 4: forward given and
  sample, then two updates.
Forward outputs and the seven update statistics are stored whole; last_grad, params and Adam's m / v after
each update as a SHA-256 and a float64 sum per tensor of the layout (in the layout's tensor order), so a
mismatch names the tensor.

Recording (once, never from the code under test): with PPO_HIP_LIB naming the parent commit's
libppo_hip.so and PYTHONPATH=ppo.cpp_amd:tests,  python tests/test_gpu_carla_bits.py OUT.npz  writes the
fixture."""
import hashlib
import os
import sys

import numpy as np
import pytest

import carla_inputs as CI

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")  # carla_ln_ref imports it
ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

import carla_ln_ref as LR  # noqa: E402
from test_gpu_carla_ln_agent import ARCHS  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "carla_bits_parent", "bits.npz")
OUTS = ("action", "logprob", "entropy", "value", "alpha", "beta")
STATS = ("pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "grad_norm")
VECTORS = ("last_grad", "params", "adam_m", "adam_v")
HYPER = dict(lr=3e-4, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, adam_eps=1e-5)
# name -> (arch options, max_batch, n, forward modes, updates)
CASES = {"default_fwd_n7": ({}, 65, 7, ("given", "sample", "mean", "roach"), 0),
         "default_fwd_n65": ({}, 65, 65, ("given", "sample"), 0),
         "default_upd_n7": ({}, 65, 7, (), 2),
         "default_upd_n65": ({}, 65, 65, (), 2)}
CASES.update({f"ln_{a}": (ARCHS[a], 4, 4, ("given", "sample"), 2) for a in ("mlp", "enc", "full_nopol", "full")})


def _digests(L, flat):
    """per tensor of the layout: SHA-256 of its bytes [ntensors, 32] and its float64 sum [ntensors]"""
    x = [flat[L.t_off[t]:L.t_off[t] + L.t_len[t]] for t in range(L.ntensors)]
    sha = np.array([np.frombuffer(hashlib.sha256(v.tobytes()).digest(), np.uint8) for v in x])
    return sha, np.array([v.astype(np.float64).sum() for v in x])


def run_case(name):
    """what the fixture holds for one case, computed with the loaded library: {key: array}, and the tensor names"""
    arch, max_batch, n, modes, updates = CASES[name]
    ppo_amd.set_device(0)
    ag = ppo_amd.CarlaAgent(max_batch=max_batch, seed=7, **arch)
    try:
        L = ag.layout2
        ag.load_params(LR.init_params(L, CI))
        ag.load_adam(np.zeros(L.P, np.float32), np.zeros(L.P, np.float32), 0)
        bev, meas, vmeas, act = CI.inputs(n)
        rng = np.random.default_rng(3)
        extra = [rng.normal(-2.0, 0.3, n), rng.normal(0.0, 1.0, n), rng.normal(0.0, 1.0, n), rng.normal(0.0, 1.0, n)]
        d = [DeviceArray.from_numpy(bev, np.uint8)] + [DeviceArray.from_numpy(np.ascontiguousarray(x, np.float32))
                                                       for x in [meas, vmeas, act] + extra]
        res = {}
        for mode in modes:
            out = ag.forward(d[0], d[1], d[2], actions=d[3] if mode == "given" else None,
                             sample_type="sample" if mode == "given" else mode, env_base=3, step_id=5)
            for k, o in zip(OUTS, out):
                res[f"{name}/forward/{mode}/{k}"] = o.numpy()
        for i in range(updates):
            st = ag.update(*d, **HYPER)
            m, v, step = ag.adam_state()
            assert step == i + 1
            res[f"{name}/update{i}/stats"] = np.array([st[k] for k in STATS], np.float32)
            dig = [_digests(L, x) for x in (ag.last_grad(), ag.params(), m, v)]  # the order of VECTORS
            res[f"{name}/update{i}/sha256"] = np.stack([sha for sha, _ in dig])
            res[f"{name}/update{i}/sum"] = np.stack([sm for _, sm in dig])
        return res, L.tensor_names()
    finally:
        ag.close()


def record(path):
    out = {}
    for name in CASES:
        out.update(run_case(name)[0])
    np.savez_compressed(path, **out)


@pytest.fixture(scope="module")
def parent():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(CASES))
def test_bits_equal_the_parent_commits(parent, name):
    got, names = run_case(name)
    want = {k: v for k, v in parent.items() if k.startswith(name + "/")}
    assert sorted(got) == sorted(want) and want
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and g.shape == w.shape, k
        if k.endswith("/sha256") or k.endswith("/sum"):  # [vector, tensor(, 32)]: name what differs
            differs = (g.view(np.uint8).reshape(4, len(names), -1) != w.view(np.uint8).reshape(4, len(names), -1)).any(2)
            assert not differs.any(), (k, [(VECTORS[a], names[t]) for a, t in zip(*np.nonzero(differs))])
        else:
            assert g.tobytes() == w.tobytes(), (k, g, w)


if __name__ == "__main__":
    record(sys.argv[1])
