"""CPU checks of the CaRL agent's LayerNorm variants (include/ppo_carla.h ppo_carla_arch /
ppo_carla_layout2, include/ppo_pth.h ppo_carla_pth_save2 / _load2): no GPU call.

  * ppo_carla_layout2_fill's tensor table (names through ppo_carla_tensor_name, lengths, offsets,
    requires_grad) against a mirror of carla_model.h:44-192 built from torch.nn modules, for the default
    agent, use_layer_norm with and without use_layer_norm_policy_head, roach_ln alone, and both;
  * the default arch's offsets are ppo_carla_layout_fill's;
  * archives: torch.jit.load sees the same names and values, load2 round-trips, an archive of another
    arch is refused with the first missing parameter's name;
  * the refusals of ppo_carla_create2 / ppo_carla_layout2_fill happen before any HIP call;
  * tests/carla_ln_ref.py with every switch off is bitwise tests/carla_torch_ref.py (fp32), and its
    conditioning leaves no pre-ReLU value within TAU of zero."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import ppo_amd as P  # noqa: E402

import carla_ln_ref as LR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCHS = [("roach", False, True), ("roach", True, True), ("roach", True, False), ("roach_ln", False, True),
         ("roach_ln", True, True), ("roach_ln", True, False)]
NTENSORS = {("roach", False): 36, ("roach", True, True): 52, ("roach", True, False): 48, ("roach_ln", False): 48,
            ("roach_ln", True, True): 64, ("roach_ln", True, False): 60}


class Mirror(torch.nn.Module):
    """carla_model.h:35-195 in torch.nn: the same children in the same registration order"""

    def __init__(self, encoder, ln, pln, C=15, NM=8, NV=3, A=2):
        super().__init__()
        nn = torch.nn
        oc, ks, st, hw = [8, 16, 32, 64, 128, 256], [5, 5, 5, 3, 3, 3], [2, 2, 2, 2, 2, 1], [94, 45, 21, 10, 4, 2]
        layers, ic = [], C
        for i in range(6):
            layers.append(nn.Conv2d(ic, oc[i], ks[i], stride=st[i]))
            if encoder == "roach_ln":
                layers.append(nn.LayerNorm([oc[i], hw[i], hw[i]]))
            layers.append(nn.ReLU())
            ic = oc[i]
        self.cnn = nn.Sequential(*layers)

        def mlp(dims, norm, last_plain=False):
            m = []
            for k, (i, o) in enumerate(dims):
                m.append(nn.Linear(i, o))
                if last_plain and k == len(dims) - 1:
                    break
                if norm:
                    m.append(nn.LayerNorm([o]))
                m.append(nn.ReLU())
            return nn.Sequential(*m)

        self.linear = mlp([(1280, 512), (512, 256)], ln)
        self.state_linear = mlp([(NM, 256), (256, 256)], ln)
        self.value_head = mlp([(256 + NV, 256), (256, 256), (256, 1)], ln, last_plain=True)
        self.policy_head = mlp([(256, 256), (256, 256)], ln and pln)
        self.dist_mu = nn.Sequential(nn.Linear(256, A))
        self.dist_sigma = nn.Sequential(nn.Linear(256, A))
        self.action_space_high = nn.Parameter(torch.tensor(1.0), requires_grad=False)
        self.action_space_low = nn.Parameter(torch.tensor(-1.0), requires_grad=False)


@pytest.mark.parametrize("encoder,ln,pln", ARCHS)
def test_layout2_is_named_parameters_of_the_module(encoder, ln, pln):
    L = P.carla_layout2(encoder=encoder, layer_norm=ln, policy_layer_norm=pln)
    want = [(n, tuple(p.shape), p.requires_grad) for n, p in Mirror(encoder, ln, pln).named_parameters()]
    assert L.ntensors == len(want) == NTENSORS[(encoder, ln, pln) if ln else (encoder, ln)]
    assert L.tensor_names() == [n for n, _, _ in want]
    assert LR.names_and_shapes(L) == [(n, s) for n, s, _ in want]
    cur = 0
    for t, (name, shape, grad) in enumerate(want):
        assert L.t_off[t] == cur and L.t_len[t] == int(np.prod(shape, dtype=np.int64)), name
        assert bool(L.t_grad[t]) == grad, name
        cur += L.t_len[t]
    assert L.P == cur
    assert (L.arch.encoder_ln, L.arch.mlp_ln, L.arch.policy_ln) == (int(encoder == "roach_ln"), int(ln),
                                                                    int(ln and pln))
    # the named offsets point at the table's entries
    names = L.tensor_names()
    at = {n: L.t_off[t] for t, n in enumerate(names)}
    step = 3 if encoder == "roach_ln" else 2
    for i in range(6):
        assert L.conv_w[i] == at[f"cnn.{step * i}.weight"] and L.conv_b[i] == at[f"cnn.{step * i}.bias"]
        if encoder == "roach_ln":
            assert L.conv_g[i] == at[f"cnn.{step * i + 1}.weight"] and L.conv_be[i] == at[f"cnn.{step * i + 1}.bias"]
        else:
            assert L.conv_g[i] == -1 and L.conv_be[i] == -1
    s = 3 if ln else 2
    sp = 3 if (ln and pln) else 2
    for k in range(2):
        for w, b, g, be, mod, st in ((L.lin_w, L.lin_b, L.lin_g, L.lin_be, "linear", s),
                                     (L.st_w, L.st_b, L.st_g, L.st_be, "state_linear", s),
                                     (L.v_w, L.v_b, L.v_g, L.v_be, "value_head", s),
                                     (L.pi_w, L.pi_b, L.pi_g, L.pi_be, "policy_head", sp)):
            assert w[k] == at[f"{mod}.{st * k}.weight"] and b[k] == at[f"{mod}.{st * k}.bias"]
            if st == 3:
                assert g[k] == at[f"{mod}.{st * k + 1}.weight"] and be[k] == at[f"{mod}.{st * k + 1}.bias"]
            else:
                assert g[k] == -1 and be[k] == -1
    assert L.v_w[2] == at[f"value_head.{2 * s}.weight"] and L.mu_w == at["dist_mu.0.weight"]
    if encoder == "roach_ln":
        assert sum(L.t_len[t] for t, n in enumerate(names) if n.startswith("cnn.") and int(n.split(".")[1]) % 3 == 1) \
            == 253344


def test_default_arch_equals_the_first_layout():
    L1, L2 = P.carla_layout(), P.carla_layout2()
    for name, _ in P.CarlaLayout._fields_:
        a, b = getattr(L1, name), getattr(L2, name)
        if name.startswith("t_"):  # tables of different capacity: the used part
            assert list(a)[:L1.ntensors] == list(b)[:L1.ntensors], name
        elif hasattr(a, "__len__"):
            assert list(a) == list(b), name
        else:
            assert a == b, name
    assert L2.tensor_names()[2:6] == ["cnn.0.weight", "cnn.0.bias", "cnn.2.weight", "cnn.2.bias"]


def test_archive_roundtrip_and_arch_mismatch(tmp_path):
    full = P.carla_layout2(encoder="roach_ln", layer_norm=True)
    params = np.random.default_rng(3).standard_normal(full.P).astype(np.float32)
    path = tmp_path / "model_0.pth"
    P.save_carla_pth2(full, params, path)
    assert np.array_equal(P.load_carla_pth2(full, path), params)
    mod = torch.jit.load(str(path))
    sd = dict(mod.named_parameters())
    assert list(sd) == full.tensor_names()
    assert tuple(sd["cnn.1.weight"].shape) == (8, 94, 94) and tuple(sd["linear.4.bias"].shape) == (256,)
    flat = np.concatenate([t.detach().numpy().reshape(-1) for t in sd.values()])
    assert np.array_equal(flat, params)
    assert len(list(mod.cnn.children())) == 18 and len(list(mod.value_head.children())) == 7
    assert len(list(mod.policy_head.children())) == 6
    # other archs refuse it and name the first parameter they miss
    with pytest.raises(P.PPOError, match=r"cnn\.2\.weight"):
        P.load_carla_pth2(P.carla_layout2(), path)
    with pytest.raises(P.PPOError, match=r"cnn\.2\.weight"):
        P.load_carla_pth2(P.carla_layout2(layer_norm=True), path)
    with pytest.raises(P.PPOError, match=r"linear\.2\.weight"):
        P.load_carla_pth2(P.carla_layout2(encoder="roach_ln"), path)
    with pytest.raises(P.PPOError, match=r"policy_head\.2\.weight"):
        P.load_carla_pth2(P.carla_layout2(encoder="roach_ln", layer_norm=True, policy_layer_norm=False), path)
    with pytest.raises(P.PPOError, match="n != layout P"):
        out = np.empty(3, np.float32)
        P.check(P.lib().ppo_carla_pth_load2(full, os.fsencode(path), out.ctypes.data, 3))
    # and the default agent's archive is what ppo_carla_pth_save writes
    d1, d2 = P.carla_layout(), P.carla_layout2()
    pd = params[:d1.P]
    P.save_carla_pth(d1, pd, tmp_path / "a.pth")
    P.save_carla_pth2(d2, pd, tmp_path / "b.pth")
    assert np.array_equal(P.load_carla_pth(d1, tmp_path / "b.pth"), pd)
    assert np.array_equal(P.load_carla_pth2(d2, tmp_path / "a.pth"), pd)
    with pytest.raises(P.PPOError, match=r"cnn\.1\.weight"):
        P.load_carla_pth2(full, tmp_path / "a.pth")


def test_refusals_come_before_any_hip_call():
    """ppo_carla_create2 refuses what the LayerNorm agent cannot do with a message and no context before it
    touches the GPU (this machine may have none). A fresh interpreter, as test_capi_cpu does."""
    script = r'''
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import ppo_amd
lib = ppo_amd.lib()
out = []
for bev, arch, opt in ((256, (1, 0, 0), None), (192, (1, 1, 1), "tail=fused"), (192, (0, 1, 0), "tail=staged"),
                       (192, (1, 0, 0), "conv1=staged,tail=fused"), (192, (2, 0, 0), None),
                       (192, (1, 1, 1), "tail=coop")):
    cfg = ppo_amd.CarlaConfig(15, bev, bev, 8, 3, 2, 1.0, 4, 7, 0)
    a = ppo_amd.CarlaArch(*arch)
    ctx = ctypes.c_void_p()
    rc = lib.ppo_carla_create2(ctypes.byref(cfg), ctypes.byref(a), 0, opt.encode() if opt else None, ctypes.byref(ctx))
    out.append([rc, bool(ctx.value), lib.ppo_last_error().decode()])
L = ppo_amd.CarlaLayout2()
a = ppo_amd.CarlaArch(1, 0, 0)
rc = lib.ppo_carla_layout2_fill(ctypes.byref(L), 15, 256, 256, 8, 3, 2, ctypes.byref(a))
out.append([rc, False, lib.ppo_last_error().decode()])
print(json.dumps(out))
'''
    res = subprocess.run([sys.executable, "-c", script, os.path.join(ROOT, "ppo.cpp_amd")], capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    want = ["192 x 192", "tail=fused cannot be used by a LayerNorm agent",
            "tail=staged cannot be used by a LayerNorm agent",
            "tail=fused cannot be used by a LayerNorm agent", "roach_ln2 is not built", "unknown option tail=coop",
            "192 x 192"]
    assert len(got) == len(want)
    for (rc, has_ctx, err), w in zip(got, want):
        assert rc != 0 and not has_ctx and w in err, (err, w)
    with pytest.raises(P.PPOError, match="Unsupported image_encoder"):
        P.carla_layout2(encoder="roach_ln2")


@pytest.mark.parametrize("conf,msg", [({"image_encoder": "roach_ln2"}, "roach_ln2"),
                                      ({"use_positional_encoding": True}, "use_positional_encoding is not built"),
                                      ({"image_encoder": "resnet"}, "Unsupported image_encoder chosen")])
def test_inference_server_refuses_what_is_not_built(tmp_path, conf, msg):
    exe = os.path.join(ROOT, "ppo.cpp_amd", "bin", "ppo_carla_inference")
    (tmp_path / "config.json").write_text(json.dumps(dict(seed=1, **conf)))
    r = subprocess.run([exe, "--path_to_conf_file", str(tmp_path), "--ipc_path", str(tmp_path / "ipc"), "--port",
                        "6100"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and msg in r.stderr, (r.returncode, r.stderr)


def _batch(n, seed):
    import carla_inputs as CI
    rng = np.random.default_rng(seed)
    bev, meas, vmeas, act = CI.inputs(n)
    return (bev, meas, vmeas, act, (rng.standard_normal(n) * 0.2).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.standard_normal(n) * 0.1).astype(np.float32))


def test_reference_without_switches_is_carla_torch_ref():
    import carla_inputs as CI
    import carla_torch_ref as TR
    torch.set_num_threads(8)
    L1, L2 = CI.layout(), P.carla_layout2()
    p = CI.params(L1)
    assert np.array_equal(LR.init_params(L2, CI), p)
    batch = _batch(3, 1)
    a = TR.update(L1, p, *batch)
    b = LR.update(L2, p, *batch)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_conditioning_clears_the_relu_margin():
    import carla_inputs as CI
    torch.set_num_threads(8)
    L = P.carla_layout2(encoder="roach_ln", layer_norm=True)
    p = LR.init_params(L, CI)
    bev, meas, vmeas, _ = CI.inputs(3)
    assert LR.min_pre_relu_distance(L, p, bev, meas, vmeas) < LR.TAU  # 2.7 M pre-ReLU values: some are close
    q, nudged = LR.condition(L, p, bev, meas, vmeas)
    assert nudged > 0 and LR.min_pre_relu_distance(L, q, bev, meas, vmeas) >= LR.TAU
    changed = np.flatnonzero(q != p)
    bias = np.zeros(L.P, bool)
    for _, bi in LR.ln_tensor_indices(L):
        bias[L.t_off[bi]:L.t_off[bi] + L.t_len[bi]] = True
    assert bias[changed].all() and np.abs(q - p).max() < 1e-2  # only LayerNorm biases moved, slightly
