"""GPU parity of the CaRL agent's LayerNorm variants (ppo_carla_create2 with a ppo_carla_arch:
image_encoder "roach_ln", use_layer_norm, use_layer_norm_policy_head; carla_model.h:44-64, :113-175):
ppo_carla_forward (given actions and "mean") and ppo_carla_update against tests/carla_ln_ref.py in fp32.

Archs: use_layer_norm alone, roach_ln alone, and both with and without the policy head's LayerNorm, n = 4;
the full arch also at n = 20 (crosses a 16-row tile with a ragged rest; old_logp = the reference's log-prob
+ N(0, 0.15), so part of the batch is clipped). Two cases run n = 9 rows on an agent created for 12 (a
ragged last minibatch): the column pass of the LayerNorm backward splits 9 rows into more chunks (9 of one
row on the [16, 45, 45] layer) than it splits 12 into (6 of two rows), and its partial-sum buffer, sized
at creation, has to hold either. Parameters are conditioned (carla_ln_ref.condition: no
pre-ReLU value within 1e-4 of zero in fp64, asserted here): one ReLU on the other side of zero would move
whole upstream gradient tensors by more than any summation order does, in PyTorch's own fp32 as well.

Bars: the project's CaRL ones. Gradient per tensor relative L2 < 1e-3 and element-wise
|d| <= 2e-3 |ref| + 1e-3 rms(tensor) (test_gpu_carla_update._check_grad, over ppo_carla_layout2's tensor
table); stats rtol 1e-4 with clipfrac within one row; total norm rtol 1e-4; parameters after one Adam step
atol 2e-6; forward outputs alpha / beta / value rtol 1e-4, log-prob and entropy atol 2e-4
(test_gpu_carla.py). A second step stays finite, counts 2 Adam steps and has moments on every LayerNorm
tensor. A one-rank communicator changes no bit; the default arch through ppo_carla_create2 is bitwise
ppo_carla_create; the inference server serves a roach_ln + use_layer_norm model folder."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import carla_inputs as CI

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

import carla_ln_ref as LR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SERVER = os.path.join(ROOT, "ppo.cpp_amd", "bin", "ppo_carla_inference")
CFG = dict(clip=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, lr=3e-4, eps=1e-5)
ARCHS = {"mlp": dict(encoder="roach", layer_norm=True, policy_layer_norm=True),
         "enc": dict(encoder="roach_ln", layer_norm=False),
         "full_nopol": dict(encoder="roach_ln", layer_norm=True, policy_layer_norm=False),
         "full": dict(encoder="roach_ln", layer_norm=True, policy_layer_norm=True)}
_CACHE = {}


def _reference(arch, n):
    """conditioned parameters, the batch and the fp32 reference's results, computed once per (arch, n)"""
    key = (arch, n)
    if key in _CACHE:
        return _CACHE[key]
    torch.set_num_threads(8)
    L = ppo_amd.carla_layout2(**ARCHS[arch])
    bev, meas, vmeas, act = CI.inputs(n)
    p, nudged = LR.condition(L, LR.init_params(L, CI), bev, meas, vmeas)
    margin = LR.min_pre_relu_distance(L, p, bev, meas, vmeas)
    fwd = LR.forward(L, p, bev, meas, vmeas, act)
    rng = np.random.default_rng(100 + n)
    old_logp = (fwd["logprob"] + rng.standard_normal(n) * 0.15).astype(np.float32)
    adv, ret = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    old_v = (rng.standard_normal(n) * 0.1).astype(np.float32)
    batch = (bev, meas, vmeas, act, old_logp, adv, ret, old_v)
    upd = LR.update(L, p, *batch, **CFG)
    for a in (p, *batch, *fwd.values(), *[np.asarray(x) for x in upd]):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _CACHE[key] = dict(L=L, p=p, batch=batch, fwd=fwd, upd=upd, margin=margin, nudged=nudged)
    return _CACHE[key]


def _dev(batch):
    return [DeviceArray.from_numpy(batch[0], np.uint8)] + [DeviceArray.from_numpy(np.ascontiguousarray(x, np.float32))
                                                           for x in batch[1:]]


def _update(ag, batch):
    st = ag.update(*_dev(batch), lr=CFG["lr"], clip_coef=CFG["clip"], ent_coef=CFG["ent_coef"], vf_coef=CFG["vf_coef"],
                   max_grad_norm=CFG["max_grad_norm"], adam_eps=CFG["eps"])
    return st, ag.last_grad(), ag.params()


def _check_grad(L, names, got, ref):
    worst = (0.0, 0.0)
    for t in range(L.ntensors):
        o, n = L.t_off[t], L.t_len[t]
        g, r = got[o:o + n].astype(np.float64), ref[o:o + n].astype(np.float64)
        nr = np.linalg.norm(r)
        if nr == 0:
            assert np.abs(g).max() == 0, names[t]
            continue
        rel = np.linalg.norm(g - r) / nr
        rms = nr / np.sqrt(n)
        el = (np.abs(g - r) / (2e-3 * np.abs(r) + 1e-3 * rms)).max()
        worst = (max(worst[0], rel), max(worst[1], el))
        assert rel < 1e-3, (names[t], rel)
        assert el <= 1.0, (names[t], el)
    return worst


@pytest.mark.parametrize("arch,n,max_batch", [("mlp", 4, 4), ("enc", 4, 4), ("full_nopol", 4, 4), ("full", 4, 4),
                                              ("full", 20, 20), ("full", 9, 12), ("mlp", 9, 12)])
def test_forward_and_update_vs_reference(arch, n, max_batch):
    ref = _reference(arch, n)
    L, p, batch = ref["L"], ref["p"], ref["batch"]
    assert ref["margin"] >= LR.TAU, ref["margin"]  # the conditioning held
    ref_g, ref_st, ref_total, ref_p, _, _ = ref["upd"]
    if n == 20:
        assert 0.0 < ref_st[5] < 1.0  # some rows clipped, not all
    ppo_amd.set_device(0)
    ag = ppo_amd.CarlaAgent(max_batch=max_batch, seed=7, **ARCHS[arch])
    try:
        assert ag.layout.ntensors == L.ntensors and ag.layout.P == L.P
        assert list(ag.layout.t_off[:L.ntensors]) == list(L.t_off[:L.ntensors])
        ag.load_params(p)
        bev, meas, vmeas, act = _dev(batch)[:4]
        _, lp, ent, v, al, be = [x.numpy() for x in ag.forward(bev, meas, vmeas, actions=act)]
        f = ref["fwd"]
        np.testing.assert_allclose(al, f["alpha"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(be, f["beta"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(v, f["value"], rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(lp, f["logprob"], rtol=1e-4, atol=2e-4)
        np.testing.assert_allclose(ent, f["entropy"], rtol=1e-4, atol=2e-4)
        am, lpm, _, vm, alm, _ = [x.numpy() for x in ag.forward(bev, meas, vmeas, sample_type="mean")]
        np.testing.assert_allclose(am, f["mean_action"], rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(lpm, f["mean_logprob"], rtol=1e-4, atol=2e-4)
        np.testing.assert_array_equal(vm, v)
        np.testing.assert_array_equal(alm, al)
        # one minibatch step
        ag.load_adam(np.zeros(L.P, np.float32), np.zeros(L.P, np.float32), 0)
        st, grad, newp = _update(ag, batch)
        stats = np.array([st[k] for k in ("pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac")])
        rel, el = _check_grad(L, L.tensor_names(), grad, ref_g)
        print(f"\n{arch} n={n} of {max_batch}: nudged {ref['nudged']} margin {ref['margin']:.2e} worst grad rel-L2 {rel:.2e} "
              f"el/bar {el:.3f} |dparam| {np.abs(newp - ref_p).max():.2e} total {st['grad_norm']:.6g} vs "
              f"{ref_total:.6g}",
              end="")
        np.testing.assert_allclose(stats[:5], ref_st[:5], rtol=1e-4, atol=2e-6)
        assert abs(stats[5] - ref_st[5]) <= 1.5 / n
        np.testing.assert_allclose(st["grad_norm"], ref_total, rtol=1e-4)
        np.testing.assert_allclose(newp, ref_p, rtol=0, atol=2e-6)
        # a second step
        st2, grad2, newp2 = _update(ag, batch)
        m, vv, step = ag.adam_state()
        assert step == 2 and np.isfinite(newp2).all() and np.isfinite(grad2).all() and np.isfinite(m).all()
        assert all(np.isfinite(x) for x in st2.values())
        for gi, bi in LR.ln_tensor_indices(L):
            for t in (gi, bi):
                o, k = L.t_off[t], L.t_len[t]
                assert np.abs(m[o:o + k]).max() > 0 and vv[o:o + k].max() > 0, L.tensor_names()[t]
    finally:
        ag.close()


def test_ln_agent_refuses_the_first_layout():
    ppo_amd.set_device(0)
    ag = ppo_amd.CarlaAgent(max_batch=2, layer_norm=True)
    try:
        with pytest.raises(ppo_amd.PPOError, match="ppo_carla_get_layout2"):
            ppo_amd.check(ppo_amd.lib().ppo_carla_get_layout(ag._h, C.byref(ppo_amd.CarlaLayout())))
    finally:
        ag.close()


def test_one_rank_communicator_is_bit_identical():
    ref = _reference("full", 4)
    out = []
    for with_comm in (False, True):
        ag = ppo_amd.CarlaAgent(max_batch=4, seed=7, **ARCHS["full"])
        try:
            ag.load_params(ref["p"])
            if with_comm:
                ag.comm_init(ppo_amd.Agent.comm_unique_id(), 0, 1)
                ag.comm_broadcast_params(0)
            out.append([_update(ag, ref["batch"]) for _ in range(2)])
        finally:
            ag.close()
    for (st0, g0, p0), (st1, g1, p1) in zip(*out):
        np.testing.assert_array_equal(g0, g1)
        np.testing.assert_array_equal(p0, p1)
        assert st0 == st1


def test_default_arch_through_create2_is_bitwise_create():
    L = CI.layout()
    p = CI.params(L)
    n = 4
    rng = np.random.default_rng(3)
    bev, meas, vmeas, act = CI.inputs(n)
    batch = (bev, meas, vmeas, act, (rng.standard_normal(n) * 0.2).astype(np.float32),
             rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32),
             (rng.standard_normal(n) * 0.1).astype(np.float32))
    out = []
    for create2 in (False, True):
        ag = ppo_amd.CarlaAgent(max_batch=n, seed=7)
        try:
            if create2:  # the same configuration through ppo_carla_create2 with an all-zero arch
                ppo_amd.lib().ppo_carla_destroy(ag._h)
                ag._h = C.c_void_p()
                ppo_amd.check(ppo_amd.lib().ppo_carla_create2(C.byref(ag.cfg), C.byref(ppo_amd.CarlaArch(0, 0, 0)), 0,
                                                              None, C.byref(ag._h)))
                lay = ppo_amd.CarlaLayout()
                ppo_amd.check(ppo_amd.lib().ppo_carla_get_layout(ag._h, C.byref(lay)))
                assert bytes(lay) == bytes(ag.layout)
            ag.load_params(p)
            d = _dev(batch)
            fw = [x.numpy() for x in ag.forward(d[0], d[1], d[2], actions=d[3])]
            out.append((fw, _update(ag, batch)))
        finally:
            ag.close()
    (f0, (s0, g0, p0)), (f1, (s1, g1, p1)) = out
    for a, b in zip(f0, f1):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(g0, g1)
    np.testing.assert_array_equal(p0, p1)
    assert s0 == s1


def test_inference_server_serves_a_layer_norm_model():
    from zmtp_peer import Peer
    L = ppo_amd.carla_layout2(**ARCHS["full"])
    p = LR.init_params(L, CI)
    bev, meas, vmeas, _ = CI.inputs(2)
    with tempfile.TemporaryDirectory() as models, tempfile.TemporaryDirectory() as ipc:
        ppo_amd.save_carla_pth2(L, p, os.path.join(models, "model_0000.pth"))
        with open(os.path.join(models, "config.json"), "w") as f:
            json.dump({"seed": 1, "obs_num_channels": CI.CH, "bev_semantics_height": CI.HW, "bev_semantics_width": CI.HW,
                       "obs_num_measurements": CI.NM, "num_value_measurements": CI.NV, "beta_min_a_b_value": CI.BETA_MIN,
                       "image_encoder": "roach_ln", "use_layer_norm": True, "ports": [5555]}, f)
        port = 6003
        srv = subprocess.Popen([SERVER, "--path_to_conf_file", models, "--ipc_path", ipc, "--port", str(port)],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        try:
            agent = Peer.connect("PAIR", f"ipc://{ipc}/{port}.lock")
            assert agent.recv() == [b"Connected to eval_agent.py."]
            agent.send([b"mean"])
            answers = []
            for k in range(2):
                agent.send([b""])
                agent.send([bev[k].tobytes(), meas[k].tobytes(), vmeas[k].tobytes()])
                answers.append([np.frombuffer(x, np.float32) for x in agent.recv()])
            agent.send([b"done"])
            out, err = srv.communicate(timeout=60)
        finally:
            if srv.poll() is None:
                srv.kill()
        assert srv.returncode == 0, err
    ag = ppo_amd.CarlaAgent(1, seed=1, **ARCHS["full"])  # use_layer_norm_policy_head defaults to true
    try:
        ag.load_params(p)
        for k, got in enumerate(answers):
            a, _, _, v, al, be = ag.forward(DeviceArray.from_numpy(bev[k:k + 1]), DeviceArray.from_numpy(meas[k:k + 1]),
                                            DeviceArray.from_numpy(vmeas[k:k + 1]), sample_type="mean", step_id=k)
            for g, w in zip(got, (a.numpy()[0], v.numpy()[:1], al.numpy()[0], be.numpy()[0])):
                np.testing.assert_array_equal(g, w)
    finally:
        ag.close()
