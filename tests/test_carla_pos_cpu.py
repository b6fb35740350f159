"""CPU checks of the CaRL agent's positional encoding (include/ppo_carla.h ppo_carla_layout2_init_pos /
ppo_carla_create3, carla_model.h:38-42, :222-236): no GPU call.

  * tests/carla_pos_ref.py with the switch off is bitwise tests/carla_ln_ref.py (fp32), for the default arch
    and a LayerNorm one; with it on its input is the raw bytes next to the two grids;
  * the layout with the switch on: P grows by 8 * 2 * 25 = 400, cnn.0.weight is [8, C + 2, 5, 5], the tensor
    count, names and requires_grad are unchanged, every offset after conv_w[0] moves by 400; with the switch
    off ppo_carla_layout2_fill_pos fills ppo_carla_layout2_fill's struct byte for byte;
  * ppo_carla_debug_pos_grid is torch.linspace(-1, 1, n) bit for bit;
  * archives: a positional layout round-trips, torch reads cnn.0.weight as [8, 17, 5, 5], and an archive of
    the other channel count is refused with the tensor's name and both shapes;
  * ppo_carla_create3's refusals happen before any HIP call."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import ppo_amd as P  # noqa: E402

import carla_inputs as CI  # noqa: E402
import carla_ln_ref as LR  # noqa: E402
import carla_pos_ref as PR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCHS = [dict(), dict(layer_norm=True), dict(encoder="roach_ln"), dict(encoder="roach_ln", layer_norm=True),
         dict(encoder="roach_ln", layer_norm=True, policy_layer_norm=False)]


def _batch(n, seed):
    rng = np.random.default_rng(seed)
    bev, meas, vmeas, act = CI.inputs(n)
    return (bev, meas, vmeas, act, (rng.standard_normal(n) * 0.2).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.standard_normal(n) * 0.1).astype(np.float32))


@pytest.mark.parametrize("arch", [dict(), dict(encoder="roach_ln", layer_norm=True)], ids=["default", "full_ln"])
def test_reference_with_the_switch_off_is_carla_ln_ref(arch):
    torch.set_num_threads(8)
    L = P.carla_layout2(**arch)
    p = LR.init_params(L, CI)
    batch = _batch(2, 1)
    a = LR.update(L, p, *batch)
    b = PR.update(L, p, *batch)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    fa, fb = LR.forward(L, p, *batch[:4]), PR.forward(L, p, *batch[:4])
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k


def test_reference_input_is_raw_bytes_and_the_two_grids():
    L = P.carla_layout2(positional_encoding=True)
    bev = CI.inputs(2)[0]
    x = PR.net_input(L, bev, torch.float32)
    assert tuple(x.shape) == (2, CI.CH + 2, CI.HW, CI.HW)
    assert np.array_equal(x[:, :CI.CH].numpy(), bev.astype(np.float32)) and x[:, :CI.CH].max() > 200  # not / 255
    lin = torch.linspace(-1, 1, CI.HW).numpy()
    assert np.array_equal(x[1, CI.CH].numpy(), np.repeat(lin[:, None], CI.HW, 1))      # constant along a row
    assert np.array_equal(x[0, CI.CH + 1].numpy(), np.repeat(lin[None, :], CI.HW, 0))  # constant along a column


@pytest.mark.parametrize("arch", ARCHS, ids=lambda a: "-".join(f"{k}={v}" for k, v in a.items()) or "default")
def test_layout_with_and_without_the_switch(arch):
    off, on = P.carla_layout2(**arch), P.carla_layout2(positional_encoding=True, **arch)
    assert on.P == off.P + 400 and on.C == off.C == 15
    assert list(on.conv_ic) == [17] + list(off.conv_ic)[1:] and off.conv_ic[0] == 15
    assert on.ntensors == off.ntensors and on.tensor_names() == off.tensor_names()
    assert list(on.t_grad) == list(off.t_grad)
    names = on.tensor_names()
    k0 = names.index("cnn.0.weight")
    assert on.t_off[k0] == off.t_off[k0] == on.conv_w[0] and on.t_len[k0] == 8 * 17 * 25 and off.t_len[k0] == 8 * 15 * 25
    for t in range(on.ntensors):
        assert on.t_off[t] == off.t_off[t] + (400 if t > k0 else 0), names[t]
        assert on.t_len[t] == off.t_len[t] + (400 if t == k0 else 0), names[t]
    # every named offset after conv_w[0] moves by 400 (-1 stays -1); shapes and the arch do not move
    for name, _ in P.CarlaLayout2._fields_:
        a, b = getattr(off, name), getattr(on, name)
        if name in ("P", "conv_ic", "t_off", "t_len") or name == "arch":
            continue
        if isinstance(a, int):
            want = a + 400 if name in ("mu_w", "mu_b", "sg_w", "sg_b") else a
            assert b == want, name
        elif name.endswith(("_w", "_b", "_g", "_be")):
            for i, (x, y) in enumerate(zip(a, b)):
                assert y == (x if x < 0 or (name == "conv_w" and i == 0) else x + 400), (name, i)
        else:
            assert list(a) == list(b), name
    assert bytes(on.arch) == bytes(off.arch)
    assert PR.names_and_shapes(on)[k0] == ("cnn.0.weight", (8, 17, 5, 5))
    # switch off: the exported fill_pos is fill, byte for byte (both into 0xAB-filled structs)
    lib = P.lib()
    a = P.carla_arch(arch.get("encoder", "roach"), arch.get("layer_norm", False), arch.get("policy_layer_norm", True))
    s1, s2 = P.CarlaLayout2(), P.CarlaLayout2()
    C.memset(C.byref(s1), 0xAB, C.sizeof(s1))
    C.memset(C.byref(s2), 0xAB, C.sizeof(s2))
    P.check(lib.ppo_carla_layout2_fill(C.byref(s1), 15, 192, 192, 8, 3, 2, C.byref(a)))
    P.check(lib.ppo_carla_layout2_fill_pos(C.byref(s2), 15, 192, 192, 8, 3, 2, C.byref(a), 0))
    assert bytes(s1) == bytes(s2)


@pytest.mark.parametrize("n", [2, 3, 160, 192, 256])
def test_grid_is_torch_linspace_bitwise(n):
    got = P.carla_pos_grid(n)
    want = torch.linspace(-1, 1, n).numpy()
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_archive_roundtrip_and_channel_mismatch(tmp_path):
    pos, plain = P.carla_layout2(positional_encoding=True), P.carla_layout2()
    params = np.random.default_rng(5).standard_normal(pos.P).astype(np.float32)
    path = tmp_path / "model_pos.pth"
    P.save_carla_pth2(pos, params, path)
    assert np.array_equal(P.load_carla_pth2(pos, path), params)
    sd = dict(torch.jit.load(str(path)).named_parameters())
    assert list(sd) == pos.tensor_names()
    assert tuple(sd["cnn.0.weight"].shape) == (8, 17, 5, 5) and tuple(sd["cnn.2.weight"].shape) == (16, 8, 5, 5)
    w0 = params[pos.conv_w[0]:pos.conv_w[0] + 8 * 17 * 25].reshape(8, 17, 5, 5)
    assert np.array_equal(sd["cnn.0.weight"].detach().numpy(), w0)
    # the Adam archive serves the layout unchanged
    m, v = params * 0.5, params * params
    P.save_carla_adam_pth2(pos, m, v, 3, 3e-4, 1e-5, tmp_path / "opt.pth")
    got = P.load_carla_adam_pth2(pos, tmp_path / "opt.pth")
    assert np.array_equal(got[0][2:], m[2:]) and np.array_equal(got[1][2:], v[2:]) and got[2] == 3  # [0, 2): no grad
    # the other channel count is refused: the tensor's name and both shapes
    with pytest.raises(P.PPOError, match=r"cnn\.0\.weight.*\[8, 17, 5, 5\].*\[8, 15, 5, 5\]"):
        P.load_carla_pth2(plain, path)
    P.save_carla_pth2(plain, params[:plain.P], tmp_path / "model_plain.pth")
    with pytest.raises(P.PPOError, match=r"cnn\.0\.weight.*\[8, 15, 5, 5\].*\[8, 17, 5, 5\]"):
        P.load_carla_pth2(pos, tmp_path / "model_plain.pth")


def test_create3_refusals_come_before_any_hip_call():
    """A fresh interpreter on a machine that may have no GPU, as test_carla_ln_cpu does for ppo_carla_create2."""
    script = r'''
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import ppo_amd
lib = ppo_amd.lib()
out = []
for bev, arch, pos, opt in ((192, (0, 0, 0), 2, None), (192, (0, 0, 0), -1, None), (192, (1, 1, 1), 1, "tail=fused"),
                            (256, (1, 0, 0), 1, None), (192, (2, 0, 0), 1, None), (192, (0, 0, 0), 1, "conv1=tiled")):
    cfg = ppo_amd.CarlaConfig(15, bev, bev, 8, 3, 2, 1.0, 4, 7, 0)
    a = ppo_amd.CarlaArch(*arch)
    ctx = ctypes.c_void_p()
    rc = lib.ppo_carla_create3(ctypes.byref(cfg), ctypes.byref(a), pos, 0, opt.encode() if opt else None,
                               ctypes.byref(ctx))
    out.append([rc, bool(ctx.value), lib.ppo_last_error().decode()])
L = ppo_amd.CarlaLayout2()
a = ppo_amd.CarlaArch(0, 0, 0)
rc = lib.ppo_carla_layout2_fill_pos(ctypes.byref(L), 15, 192, 192, 8, 3, 2, ctypes.byref(a), 3)
out.append([rc, False, lib.ppo_last_error().decode()])
print(json.dumps(out))
'''
    res = subprocess.run([sys.executable, "-c", script, os.path.join(ROOT, "ppo.cpp_amd")], capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    want = ["pos_enc must be 0 or 1", "pos_enc must be 0 or 1", "tail=fused cannot be used by a LayerNorm agent",
            "192 x 192", "roach_ln2 is not built", "unknown option conv1=tiled", "pos_enc must be 0 or 1"]
    assert len(got) == len(want)
    for (rc, has_ctx, err), w in zip(got, want):
        assert rc != 0 and not has_ctx and w in err, (err, w)
