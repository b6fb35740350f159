"""GPU tests of the CaRL agent's positional encoding (ppo_carla_create3 with pos_enc = 1; carla_model.h:38-42,
:222-236; include/ppo_carla.h, ppo_carla_pos.hip).

Hooks (OC 8, C 3, K 5, S 2 on a 37 x 53 input, so 17 x 25 outputs: not square, a swapped height and width
shows):
  * ppo_carla_debug_pos_bias: rowb[oc, oy] + colb[oc, ox] against the fp64 conv2d of the two grids; per oc
    |d| <= 64 * 2^-24 * sum |W[oc, C.., :, :]| (50 products with |grid| <= 1 plus the table roundings);
  * ppo_carla_debug_pos_wgrad (n = 3, n = 20, n = 9 with buffers made for 12) against fp64; per element
    |d| <= m * 2^-24 * sum |dZ[:, oc]| with m = n OH OW + K (the summation bound; an index error is O(1)
    relative); dW[oc, 0, ky, :] are bitwise equal, dW[oc, 1, :, kx] too; two calls give the same bits.

Agent against tests/carla_pos_ref.py in fp32: roach + pos and roach_ln + pos at n = 4, the full LayerNorm arch
+ pos at n = 4, n = 20 and n = 9 on an agent made for 12. Parameters: carla_ln_ref.init_params over the
positional layout, conditioned (TAU = 1e-4, margin asserted); for roach + pos the image channels of
cnn.0.weight are multiplied by 1 / 255, so the un-normalised input gives activations of the usual size. Bars:
the project's CaRL ones (test_gpu_carla_ln_agent.py): alpha / beta / value rtol 1e-4, log-prob and entropy atol
2e-4, gradient per tensor rel-L2 < 1e-3 and |d| <= 2e-3 |ref| + 1e-3 rms, stats rtol 1e-4 with clipfrac within
one row, total norm rtol 1e-4, parameters after one Adam step atol 2e-6. grad[cnn.0.weight][:, C:] is held to
the two gradient bars ON ITS OWN (own norm and rms): it is ~0.1 % of that tensor's gradient norm, because the
raw-byte channels carry a factor 255, so the whole-tensor bar would pass with the slice entirely wrong.
Asserted on the CPU first: the fp32 reference is within a third of every bar of the fp64 one, and the
reference forward with the positional weights zeroed differs by more than 100 x the forward bar (rtol 1e-4 of
alpha / beta / value), so that the forward comparison has teeth. That second condition holds for roach + pos
(0.10) but cannot hold for the LayerNorm encoders on these parameters: their cnn.0 sees raw bytes, the image
channels give pre-activations of ~70 against ~0.3 from the two planes, and the LayerNorm after cnn.0 divides
both by the row's deviation. Measured on the CPU reference: zeroing the planes' weights moves alpha / beta /
value by at most 1.2e-3 (roach_ln + pos, n = 4) and 3.1e-3 (full arch + pos, n = 4) relative, 5 to 30 x the
bar. So for those cases the test asserts what the comparison needs (a forward without the positional term fails
it at TWICE its tolerances: the device's own deviation was just bounded by a third of them), and two more
cases carry the 100 x condition for the LayerNorm encoders: "enc_s" / "full_s", the same archs at n = 4 with
the image channels of cnn.0.weight multiplied by 1 / 255 as in the roach case, where the planes are a large
part of cnn.0's output. In the unscaled LayerNorm cases the forward comparison is therefore only 5 to 30 x its
bar away from not seeing the planes: the scaled cases are the real forward check of the positional term for
the LayerNorm encoders, and the gradient slice's own bars are the check of its backward in every case.

conv1=generic (and conv1=staged) against the default packed path at the agreement of
test_gpu_carla.py's packed-vs-generic test (outputs rtol 2e-5 / atol 2e-6, gradients rel-L2 1e-5).
Bitwise: the three tail modes on a positional agent; ppo_carla_create3(pos_enc = 0) is ppo_carla_create2; a one-rank communicator changes nothing; a lane
act is ppo_carla_rollout_act(step, env, env + 1), the training after either collection gives the same
parameters, and a rerun gives the same bits."""
import ctypes as C
import threading

import numpy as np
import pytest

import carla_inputs as CI

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

import carla_pos_ref as PR  # noqa: E402
import test_gpu_carla_lanes as TL  # noqa: E402  (parameter / observation / serial-collection helpers)

CFG = dict(clip=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, lr=3e-4, eps=1e-5)
ARCHS = {"roach": dict(encoder="roach", layer_norm=False),
         "enc": dict(encoder="roach_ln", layer_norm=False),
         "full": dict(encoder="roach_ln", layer_norm=True, policy_layer_norm=True)}
ARCHS["enc_s"], ARCHS["full_s"] = ARCHS["enc"], ARCHS["full"]
OC, CH, K, S, IH, IW = 8, 3, 5, 2, 37, 53
OH, OW = (IH - K) // S + 1, (IW - K) // S + 1
U = 2.0 ** -24
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _grids64(n):
    g0, g1 = torch.meshgrid(torch.linspace(-1, 1, IH), torch.linspace(-1, 1, IW), indexing="ij")
    return torch.stack([g0, g1]).double().unsqueeze(0).expand(n, -1, -1, -1)


# ------------------------------------------------------------------------------------------------
# hooks
# ------------------------------------------------------------------------------------------------
def test_pos_bias_tables_vs_fp64_conv_of_the_grids():
    assert (OH, OW) == (17, 25)
    ppo_amd.set_device(0)
    rng = np.random.default_rng(11)
    W = rng.uniform(-0.2, 0.2, (OC, CH + 2, K, K)).astype(np.float32)
    rowb, colb = ppo_amd.carla_pos_bias(DeviceArray.from_numpy(W), OC, CH + 2, CH, K, S, IH, IW)
    rowb, colb = rowb.numpy().astype(np.float64), colb.numpy().astype(np.float64)
    assert rowb.shape == (OC, OH) and colb.shape == (OC, OW)
    ref = torch.nn.functional.conv2d(_grids64(1), torch.tensor(W[:, CH:]).double(), stride=S)[0].numpy()
    got = rowb[:, :, None] + colb[:, None, :]
    d = np.abs(got - ref).reshape(OC, -1).max(1)
    bound = 64 * U * np.abs(W[:, CH:].astype(np.float64)).reshape(OC, -1).sum(1)
    print(f"\nmax |d| / bound per oc: {(d / bound).max():.3f}", end="")
    assert (d <= bound).all(), (d, bound)
    assert np.abs(ref).max() > 0.1  # the tables are not small beside the bound (1e-5)


@pytest.mark.parametrize("n,max_n", [(3, 3), (20, 20), (9, 12)])
def test_pos_wgrad_vs_fp64(n, max_n):
    ppo_amd.set_device(0)
    rng = np.random.default_rng(100 + n)
    dz = rng.standard_normal((n, OC, OH, OW)).astype(np.float32)
    w = torch.zeros(OC, 2, K, K, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.conv2d(_grids64(n), w, stride=S) * torch.tensor(dz).double()).sum().backward()
    ref = w.grad.numpy()
    d_dz = DeviceArray.from_numpy(dz)
    got = ppo_amd.carla_pos_wgrad(d_dz, n, OC, K, S, IH, IW, max_n=max_n).numpy()
    again = ppo_amd.carla_pos_wgrad(d_dz, n, OC, K, S, IH, IW, max_n=max_n).numpy()
    assert got.shape == (OC, 2, K, K)
    bound = (n * OH * OW + K) * U * np.abs(dz.astype(np.float64)).sum((0, 2, 3))
    d = np.abs(got.astype(np.float64) - ref).reshape(OC, -1).max(1)
    print(f"\nmax |d| / bound per oc: {(d / bound).max():.4f}", end="")
    assert (d <= bound).all(), (d, bound)
    # the bound is loose (it grows with n^2, the entries with sqrt(n)) but still below the entries themselves:
    # an index error, O(1) relative, lands outside it
    assert (np.abs(ref).reshape(OC, -1).max(1) > 4 * bound).all()
    b = _bits(got)
    assert (b[:, 0] == b[:, 0, :, :1]).all()  # dW[oc, 0, ky, :]: one value per ky
    assert (b[:, 1] == b[:, 1, :1, :]).all()  # dW[oc, 1, :, kx]: one value per kx
    np.testing.assert_array_equal(b, _bits(again))


# ------------------------------------------------------------------------------------------------
# the agent against the reference
# ------------------------------------------------------------------------------------------------
def _pos_slice(L, flat):
    w = flat[L.conv_w[0]:L.conv_w[0] + L.t_len[2]].reshape(L.conv_oc[0], L.conv_ic[0], -1)
    return w[:, L.C:].reshape(-1)


def _grad_worst(L, got, ref, extra=None):
    """(worst per-tensor rel-L2, worst element / bar) over the tensor table and the positional slice"""
    pairs = [(L.tensor_names()[t], got[L.t_off[t]:L.t_off[t] + L.t_len[t]], ref[L.t_off[t]:L.t_off[t] + L.t_len[t]])
             for t in range(L.ntensors)]
    pairs.append(("cnn.0.weight[:, C:]", _pos_slice(L, got), _pos_slice(L, ref)))
    worst = [0.0, 0.0, "", ""]
    for name, g, r in pairs:
        g, r = g.astype(np.float64), r.astype(np.float64)
        nr = np.linalg.norm(r)
        if nr == 0:
            assert np.abs(g).max() == 0, name
            continue
        rel = np.linalg.norm(g - r) / nr
        el = (np.abs(g - r) / (2e-3 * np.abs(r) + 1e-3 * nr / np.sqrt(r.size))).max()
        if rel > worst[0]:
            worst[0], worst[2] = rel, name
        if el > worst[1]:
            worst[1], worst[3] = el, name
    return worst


FWD_BARS = (("alpha", 1e-4, 1e-5), ("beta", 1e-4, 1e-5), ("value", 1e-4, 2e-5), ("logprob", 1e-4, 2e-4),
            ("entropy", 1e-4, 2e-4))
SCALED = ("roach", "enc_s", "full_s")  # image channels of cnn.0.weight times 1 / 255


def _reference(arch, n):
    """conditioned parameters, the batch, the fp32 and fp64 references, and the CPU-side preconditions"""
    key = (arch, n)
    if key in _CACHE:
        return _CACHE[key]
    torch.set_num_threads(8)
    L = ppo_amd.carla_layout2(positional_encoding=True, **ARCHS[arch])
    bev, meas, vmeas, act = CI.inputs(n)
    p = PR.init_params(L, CI)
    if arch in SCALED:
        p = PR.scale_image_filters(L, p, 1.0 / 255.0)
    p, nudged = PR.condition(L, p, bev, meas, vmeas)
    margin = PR.min_pre_relu_distance(L, p, bev, meas, vmeas)
    assert margin >= PR.TAU, margin  # the conditioning held (inf without LayerNorm)
    fwd = PR.forward(L, p, bev, meas, vmeas, act)
    rng = np.random.default_rng(100 + n)
    old_logp = (fwd["logprob"] + rng.standard_normal(n) * 0.15).astype(np.float32)
    adv, ret = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    old_v = (rng.standard_normal(n) * 0.1).astype(np.float32)
    batch = (bev, meas, vmeas, act, old_logp, adv, ret, old_v)
    upd = PR.update(L, p, *batch, **CFG)
    # --- the fp32 reference is within a third of every bar of the fp64 one
    f64 = PR.forward(L, p, bev, meas, vmeas, act, dtype=torch.float64)
    u64 = PR.update(L, p, *batch, dtype=torch.float64, **CFG)
    third = 1.0 / 3.0
    for k, rt, at in FWD_BARS:
        np.testing.assert_allclose(fwd[k], f64[k], rtol=rt * third, atol=at * third, err_msg=k)
    rel, el, rel_at, el_at = _grad_worst(L, upd[0], u64[0])
    assert rel < 1e-3 * third and el <= third, (rel, rel_at, el, el_at)
    np.testing.assert_allclose(upd[1][:5], u64[1][:5], rtol=1e-4 * third, atol=2e-6 * third)
    assert upd[1][5] == u64[1][5]
    np.testing.assert_allclose(upd[2], u64[2], rtol=1e-4 * third)
    np.testing.assert_allclose(upd[3], u64[3], rtol=0, atol=2e-6 * third)
    # --- teeth: without the positional weights the forward moves by more than 100 x its bar (module docstring)
    fz = PR.forward(L, p, bev, meas, vmeas, act, zero_pos=True)
    teeth = max(float((np.abs(fz[k] - fwd[k]) / np.abs(fwd[k])).max()) for k in ("alpha", "beta", "value"))
    if arch in SCALED:
        assert teeth > 100 * 1e-4, teeth
    assert any(not np.allclose(fz[k], fwd[k], rtol=2 * rt, atol=2 * at) for k, rt, at in FWD_BARS), teeth
    assert (_pos_slice(L, upd[0]) != 0).all()  # every positional weight has a gradient to find
    for a in (p, *batch, *fwd.values(), *[np.asarray(x) for x in upd]):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _CACHE[key] = dict(L=L, p=p, batch=batch, fwd=fwd, upd=upd, margin=margin, nudged=nudged, teeth=teeth,
                       f32_vs_f64=(rel, el))
    return _CACHE[key]


def _dev(batch):
    return [DeviceArray.from_numpy(batch[0], np.uint8)] + [DeviceArray.from_numpy(np.ascontiguousarray(x, np.float32))
                                                           for x in batch[1:]]


def _update(ag, batch):
    st = ag.update(*_dev(batch), lr=CFG["lr"], clip_coef=CFG["clip"], ent_coef=CFG["ent_coef"], vf_coef=CFG["vf_coef"],
                   max_grad_norm=CFG["max_grad_norm"], adam_eps=CFG["eps"])
    return st, ag.last_grad(), ag.params()


@pytest.mark.parametrize("arch,n,max_batch", [("roach", 4, 4), ("enc", 4, 4), ("full", 4, 4), ("full", 20, 20),
                                              ("full", 9, 12), ("enc_s", 4, 4), ("full_s", 4, 4)])
def test_forward_and_update_vs_reference(arch, n, max_batch):
    ref = _reference(arch, n)
    L, p, batch = ref["L"], ref["p"], ref["batch"]
    ref_g, ref_st, ref_total, ref_p, _, _ = ref["upd"]
    if n == 20:
        assert 0.0 < ref_st[5] < 1.0  # some rows clipped, not all
    ppo_amd.set_device(0)
    ag = ppo_amd.CarlaAgent(max_batch=max_batch, seed=7, positional_encoding=True, **ARCHS[arch])
    try:
        assert ag.layout2.conv_ic[0] == CI.CH + 2 and ag.layout2.C == CI.CH
        assert bytes(ag.layout2) == bytes(L)
        with pytest.raises(ppo_amd.PPOError, match="ppo_carla_get_layout2"):
            ppo_amd.check(ppo_amd.lib().ppo_carla_get_layout(ag._h, C.byref(ppo_amd.CarlaLayout())))
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
        rel, el, rel_at, el_at = _grad_worst(L, grad, ref_g)
        gp, rp = _pos_slice(L, grad).astype(np.float64), _pos_slice(L, ref_g).astype(np.float64)
        print(f"\n{arch}+pos n={n} of {max_batch}: nudged {ref['nudged']} margin {ref['margin']:.2e} teeth "
              f"{ref['teeth']:.2e} f32-vs-f64 {ref['f32_vs_f64'][0]:.1e}/{ref['f32_vs_f64'][1]:.3f} worst grad rel-L2 "
              f"{rel:.2e} ({rel_at}) el/bar {el:.3f} ({el_at}) pos slice rel-L2 "
              f"{np.linalg.norm(gp - rp) / np.linalg.norm(rp):.2e} |dparam| {np.abs(newp - ref_p).max():.2e} total "
              f"{st['grad_norm']:.6g} vs {ref_total:.6g}", end="")
        assert rel < 1e-3, (rel_at, rel)
        assert el <= 1.0, (el_at, el)
        np.testing.assert_allclose(stats[:5], ref_st[:5], rtol=1e-4, atol=2e-6)
        assert abs(stats[5] - ref_st[5]) <= 1.5 / n
        np.testing.assert_allclose(st["grad_norm"], ref_total, rtol=1e-4)
        np.testing.assert_allclose(newp, ref_p, rtol=0, atol=2e-6)
        # a second step: finite, two Adam steps, every positional weight has a first moment
        st2, grad2, newp2 = _update(ag, batch)
        m, vv, step = ag.adam_state()
        assert step == 2 and np.isfinite(newp2).all() and np.isfinite(grad2).all() and np.isfinite(m).all()
        assert all(np.isfinite(x) for x in st2.values())
        assert _pos_slice(L, m).size == 400 and (_pos_slice(L, m) != 0).all() and (_pos_slice(L, vv) > 0).all()
    finally:
        ag.close()


@pytest.mark.parametrize("arch", ["roach", "full"])
def test_generic_and_staged_conv1_match_the_default_path(arch):
    ref = _reference(arch, 4)
    L, batch = ref["L"], ref["batch"]
    outs = []
    for opt in (None, "conv1=generic", "conv1=staged", "conv1_mfma=f32"):
        ag = ppo_amd.CarlaAgent(max_batch=4, seed=7, positional_encoding=True, options=opt, **ARCHS[arch])
        try:
            ag.load_params(ref["p"])
            d = _dev(batch)
            fw = [x.numpy() for x in ag.forward(d[0], d[1], d[2], actions=d[3])]
            outs.append((opt, fw, _update(ag, batch)[1]))
        finally:
            ag.close()
    _, f0, g0 = outs[0]
    for opt, f1, g1 in outs[1:]:
        for a, b in zip(f0, f1):
            np.testing.assert_allclose(b, a, rtol=2e-5, atol=2e-6, err_msg=opt)
        for t in list(range(2, L.ntensors)) + [-1]:
            x, y = (_pos_slice(L, g0), _pos_slice(L, g1)) if t < 0 else \
                (g0[L.t_off[t]:L.t_off[t] + L.t_len[t]], g1[L.t_off[t]:L.t_off[t] + L.t_len[t]])
            rel = np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(x.astype(np.float64))
            assert rel < 1e-5, (opt, t, rel)


# ------------------------------------------------------------------------------------------------
# equalities, all bitwise
# ------------------------------------------------------------------------------------------------
def test_tail_modes_are_bitwise_equal_on_a_positional_agent():
    """conv1 is outside the MLP tail: tail=staged (default), tail=fused and tail=layers give the same bits"""
    ref = _reference("roach", 4)
    outs = []
    for opt in (None, "tail=fused", "tail=layers"):
        ag = ppo_amd.CarlaAgent(max_batch=4, seed=7, positional_encoding=True, options=opt, **ARCHS["roach"])
        try:
            ag.load_params(ref["p"])
            d = _dev(ref["batch"])
            outs.append([x.numpy() for x in ag.forward(d[0], d[1], d[2], actions=d[3])] +
                        [x.numpy() for x in ag.forward(d[0], d[1], d[2], sample_type="sample", env_base=3, step_id=5)])
        finally:
            ag.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            np.testing.assert_array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("arch", [dict(), ARCHS["full"]], ids=["default", "full_ln"])
def test_create3_without_the_switch_is_create2(arch):
    L = ppo_amd.carla_layout2(**arch)
    p = PR.init_params(L, CI)
    n = 4
    rng = np.random.default_rng(3)
    bev, meas, vmeas, act = CI.inputs(n)
    batch = (bev, meas, vmeas, act, (rng.standard_normal(n) * 0.2).astype(np.float32),
             rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32),
             (rng.standard_normal(n) * 0.1).astype(np.float32))
    out = []
    for create3 in (False, True):
        ag = ppo_amd.CarlaAgent(max_batch=n, seed=7, **arch)
        try:
            ppo_amd.lib().ppo_carla_destroy(ag._h)
            ag._h = C.c_void_p()
            if create3:
                ppo_amd.check(ppo_amd.lib().ppo_carla_create3(C.byref(ag.cfg), C.byref(ag.arch), 0, 0, None,
                                                              C.byref(ag._h)))
            else:
                ppo_amd.check(ppo_amd.lib().ppo_carla_create2(C.byref(ag.cfg), C.byref(ag.arch), 0, None, C.byref(ag._h)))
            lay = ppo_amd.CarlaLayout2()
            ppo_amd.check(ppo_amd.lib().ppo_carla_get_layout2(ag._h, C.byref(lay)))
            assert bytes(lay) == bytes(L)
            ag.load_params(p)
            d = _dev(batch)
            fw = [x.numpy() for x in ag.forward(d[0], d[1], d[2], actions=d[3])]
            out.append((fw, _update(ag, batch)))
        finally:
            ag.close()
    (f0, (s0, g0, p0)), (f1, (s1, g1, p1)) = out
    for a, b in zip(f0, f1):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    np.testing.assert_array_equal(_bits(g0), _bits(g1))
    np.testing.assert_array_equal(_bits(p0), _bits(p1))
    assert s0 == s1


def test_one_rank_communicator_is_bit_identical():
    ref = _reference("full", 4)
    out = []
    for with_comm in (False, True):
        ag = ppo_amd.CarlaAgent(max_batch=4, seed=7, positional_encoding=True, **ARCHS["full"])
        try:
            ag.load_params(ref["p"])
            if with_comm:
                ag.comm_init(ppo_amd.Agent.comm_unique_id(), 0, 1)
                ag.comm_broadcast_params(0)
            out.append([_update(ag, ref["batch"]) for _ in range(2)])
        finally:
            ag.close()
    for (st0, g0, p0), (st1, g1, p1) in zip(*out):
        np.testing.assert_array_equal(_bits(g0), _bits(g1))
        np.testing.assert_array_equal(_bits(p0), _bits(p1))
        assert st0 == st1
    assert (_pos_slice(ref["L"], out[1][0][1]) != 0).all()  # the rank average covers the positional weights


def _collect_and_train(lanes):
    """E = 2, T = 2 on a positional agent: collect serially or through one lane per env (a thread each),
    GAE, one rollout_train (1 epoch x 2 minibatches of 2 rows); the stored collection and the parameters"""
    t_steps, e_envs = 2, 2
    ag = ppo_amd.CarlaAgent(max_batch=2, seed=7, positional_encoding=True)
    ro = ppo_amd.CarlaRollout(ag, t_steps, e_envs, 1, 2, 0.99, 0.95, seed=5)
    try:
        L = ag.layout2
        p_init = PR.scale_image_filters(L, TL._params(L, 3), 1.0 / 255.0)
        ag.load_params(p_init)
        obs = TL._observations(20, t_steps, e_envs, 15, 192)
        if lanes:
            ln = [ro.lane() for _ in range(e_envs)]
            acts = np.zeros((t_steps, e_envs, 2), np.float32)
            errors = []

            def work(e):
                try:
                    for t in range(t_steps):
                        acts[t, e] = ln[e].act(t, e, obs["bev"][t, e], obs["meas"][t, e], obs["vmeas"][t, e],
                                               obs["done"][t, e])
                        ln[e].reward(t, e, obs["reward"][t, e])
                    ln[e].sync()
                except Exception as ex:  # noqa: BLE001
                    errors.append(repr(ex))

            threads = [threading.Thread(target=work, args=(e,)) for e in range(e_envs)]
            for th in threads:
                th.start()
            for th in threads:
                th.join()
            assert not errors, errors
        else:
            acts = TL._serial(ro, obs, t_steps, e_envs)
        stored = {k: ro.buffer(k).numpy().copy() for k in TL.STORED}
        ro.gae(*[DeviceArray.from_numpy(obs[k][t_steps]) for k in ("bev", "meas", "vmeas", "done")])
        ro.train(lr=1e-3, want_stats=False)
        return acts, stored, ag.params(), p_init
    finally:
        ro.close(), ag.close()


def test_lane_acts_equal_serial_acts_and_rerun_is_bitwise():
    ppo_amd.set_device(0)
    runs = [_collect_and_train(False), _collect_and_train(True), _collect_and_train(False), _collect_and_train(True)]
    acts0, stored0, p0, p_init = runs[0]
    assert np.isfinite(acts0).all() and len(np.unique(acts0)) > 4 and np.isfinite(p0).all()
    assert not np.array_equal(p0[2:], p_init[2:])
    for acts, stored, p, _ in runs[1:]:
        np.testing.assert_array_equal(_bits(acts), _bits(acts0))
        for k in TL.STORED:
            np.testing.assert_array_equal(stored[k].view(np.uint8), stored0[k].view(np.uint8), err_msg=k)
        np.testing.assert_array_equal(_bits(p), _bits(p0))
