"""Every kernel copy of the Beta policy head against its fp64 restatement (tests/beta_ref.py) over the
concentrations a policy can reach: exactly 1 (softplus underflows), 1 + 3e-7, the thresholds of the special
functions (the Stirling shift's x < 6, ATen digamma's x < 10 and x == 10, softplus's 20), and the tens to a
thousand of a trained policy; at given actions on the clamps (lo, hi, beyond both, s = 1e-7, the largest
sample 1 - 2^-24). The bound scales with the addends (beta_ref's module docstring); its constants are measured
on the reference's fp32 arithmetic in tests/test_beta_ref_cpu.py.

Copies reached: k_act3 with one and two input blocks, k_act2 (hidden 64), k_carla_tail,
k_carla_head; k_rollout + k_beta_logp, k_rollout_v + k_beta_logp, the per-step ppo_rollout_act, k_eval;
k_upd's 8-lane group (A = 3, 6, 8) as bx6 / fp32 16x16x4 / k_upd32 / its mixed form, k_fwdbwd at hidden 256
and 64, k_carla_head_bwd. Not reached through the C-ABI: k_upd's LDS item path for A > 8 (below), k_rollout
with log-probs in the loop (ppo_rollout_synth always defers them for this agent).

Behaviour the reference shares and the tests expect: log-prob -inf at action = hi with beta > 1 (s = 1,
log 0), NaN at an action above hi (scale_action's upper clamp is 1 + 1e-7f = 1 + 2^-23, so 1 - s < 0), and at
(1e4, 1e4) an error of 2e-2 in the reference's own fp32 formula, which the bound allows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
import beta_ref as B  # noqa: E402
import oracle_lib as Orc  # noqa: E402
from ppo_amd import DeviceArray  # noqa: E402
from test_gpu_parity import fill_storage, rel  # noqa: E402

# (O, A, H): k_act3 two input blocks + k_upd 8-lane group with two idle lanes; one input block; the full
# group; hidden 64: k_act2 and k_fwdbwd. No A > 8 at hidden 256 (test_a_above_8_is_out_of_reach_at_hidden_256)
SHAPES = [(17, 6, 256), (11, 3, 256), (17, 8, 256), (17, 6, 64)]
ROWS = (1, 3, 70)
E_UPD, T_UPD = 37, 3          # M = 111: a ragged last tile, whose padding rows take the kernels' !valid path
CLIP = 0.2
SETTINGS = {"logp": 0.0, "ent": 1.0, "default": 0.01}   # ent_coef; "ent" also zeroes the advantages
MODES = {"given": ppo_amd.PPO_GIVEN, "mean": ppo_amd.PPO_MEAN, "roach": ppo_amd.PPO_ROACH}

WORST = {}


def note(copy, quantity, ratio):
    """the largest error / bound per (copy, quantity), printed by the last test of the module"""
    k = (copy, quantity)
    WORST[k] = max(WORST.get(k, 0.0), float(ratio))


def make_agent(O_, A, H, E=64, T=1, ent=0.01, options=None):
    # advantage normalisation off; eager update launches (ent_coef is a launch constant of this context)
    hc = ppo_amd.HipConfig(1, O_, A, H, E, T, 1, 1, 0.99, 0.95, CLIP, ent, 0.5, 0.5, 1e-5, 0, 1, 1, 0, 1)
    return ppo_amd.Agent(hc, options=options)


def same_nonfinite(dev, ref):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    return (np.array_equal(np.isnan(dev), np.isnan(ref)) and np.array_equal(np.isneginf(dev), np.isneginf(ref))
            and not np.isposinf(dev).any())


def expand(al, be, n):
    return np.broadcast_to(al, (n, al.size)), np.broadcast_to(be, (n, be.size))


def check_forward(copy, mode, act_dev, lp, ent, al, be, act_given, names, load):
    """One forward call's outputs against beta_fp64 (al, be: the reference's fp32 concentrations [A])."""
    n = lp.shape[0]
    ala, bea = expand(al, be, n)
    if mode == "given":
        s, extra = B.scale_action(act_given), 0.0
        # the returned action is the round trip of the clamped s (test_gpu_parity.py: atol 2e-7)
        np.testing.assert_allclose(act_dev, B.unscale_action(s), rtol=0, atol=2e-7)
    else:
        s = np.broadcast_to(B.mean01(al, be) if mode == "mean" else B.roach01(al, be), (n, al.size))
        # the device's s is its own quotient of its own concentrations: two ulps of s
        extra = 2.0
        np.testing.assert_allclose(act_dev, B.unscale_action(s), rtol=1e-4, atol=2e-5)
    ref = B.beta_fp64(ala, bea, s)
    rl, re_ = ref["lp"].numpy().sum(-1), ref["ent"].numpy().sum(-1)
    bd = B.row_bounds(ref, s_ulps=extra)
    assert same_nonfinite(lp, rl), (copy, mode, load, names, lp, rl)
    assert np.isfinite(ent).all() and np.isfinite(re_).all(), (copy, mode, load)
    ok = np.isfinite(rl)
    with np.errstate(invalid="ignore"):
        el, ee = np.abs(lp - rl)[ok] / bd["lp"][ok], np.abs(ent - re_) / bd["ent"]
    if ok.any():
        note(copy, "logp", el.max())
        assert (el <= 1).all(), (copy, mode, load, names, el)
    note(copy, "entropy", ee.max())
    assert (ee <= 1).all(), (copy, mode, load, ee)


# ------------------------------------------------------------------------------------------------
# (a) forward: every act copy
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "O%d_A%d_H%d" % s)
def act_agent(request):
    O_, A, H = request.param
    ag = make_agent(O_, A, H)
    yield ag, Orc.layout_init(1, O_, A, H)
    ag.close()


@pytest.mark.parametrize("n", ROWS)
def test_forward_given_mean_roach(act_agent, n):
    """ppo_get_action_and_value in PPO_GIVEN / PPO_MEAN / PPO_ROACH over every grid load and the far point
    (1e4, 1e4): log-prob and entropy per row within the bound, the returned actions within the existing
    action bars, -inf (not NaN) at action = hi with beta > 1, NaN exactly where the reference has it."""
    ag, L = act_agent
    copy = "k_act2" if L.H == 64 else "k_act3/OP%d" % (16 if L.O <= 16 else 32)
    rng = np.random.default_rng(100 * L.O + L.A + L.H + n)
    x = DeviceArray.from_numpy(rng.standard_normal((n, L.O)).astype(np.float32))
    for load in B.grid_loads(L.A) + [[B.FAR] * L.A]:
        p, al, be = B.head_params(L, rng, [t[0] for t in load], [t[1] for t in load])
        ag.load_params(p)
        given, names = B.given_actions(al, be, n)
        for mode, m in MODES.items():
            a = DeviceArray.from_numpy(given) if mode == "given" else None
            act, lp, ent, _ = ag.get_action_and_value(x, m, a)
            check_forward(copy, mode, act.numpy(), lp.numpy(), ent.numpy(), al, be, given, names, load)


@pytest.mark.parametrize("tail", ["fused", "layers"])
def test_carla_forward_given_mean_roach(tail):
    """The CaRL agent's head (concentration softplus + beta_min, dist_mu / dist_sigma weights zeroed like
    the MLP heads): k_carla_tail (tail=fused) and k_carla_head (tail=layers) at the smallest batch of
    test_gpu_carla.py; the returned alpha / beta are the reference's concentrations to an ulp."""
    import carla_inputs as CI
    L = CI.layout()
    base = CI.params(L)
    n = 3
    bev, meas, vmeas, _ = CI.inputs(n)
    d = [DeviceArray.from_numpy(bev, np.uint8), DeviceArray.from_numpy(meas), DeviceArray.from_numpy(vmeas)]
    ag = ppo_amd.CarlaAgent(max_batch=16, seed=7, options="tail=" + tail)
    copy = "k_carla_tail" if tail == "fused" else "k_carla_head"
    try:
        for load in B.grid_loads(L.A) + [[B.FAR] * L.A]:
            p, al, be = carla_head_params(L, base, load)
            ag.load_params(p)
            for k in range(4):   # rotate the ten given-action cases through the three rows
                given, names = B.given_actions(al, be, 10)
                pick = [(3 * k + j) % 10 for j in range(n)]
                given, names = np.ascontiguousarray(given[pick]), [names[j] for j in pick]
                for mode in MODES:
                    if mode != "given" and k:
                        continue
                    out = ag.forward(*d, actions=DeviceArray.from_numpy(given) if mode == "given" else None,
                                     sample_type=mode if mode != "given" else "sample")
                    act, lp, ent, _, dal, dbe = [o.numpy() for o in out]
                    for dv, rv in ((dal, al), (dbe, be)):
                        assert (np.abs(dv - rv[None, :]) <= 2 * np.spacing(rv)[None, :]).all(), (load, dv, rv)
                    check_forward(copy, mode, act, lp, ent, al, be, given, names, load)
    finally:
        ag.close()


def carla_head_params(L, base, load):
    p = base.copy()
    ba = np.array([B.bias_of(t[0]) for t in load], np.float32)
    bb = np.array([B.bias_of(t[1]) for t in load], np.float32)
    for w, b, v in ((L.mu_w, L.mu_b, ba), (L.sg_w, L.sg_b, bb)):
        p[w:w + L.A * 256] = 0.0
        p[b:b + L.A] = v
    return p, B.conc_of_bias(ba), B.conc_of_bias(bb)   # beta_min = 1


# ------------------------------------------------------------------------------------------------
# (b) collection: every path
# ------------------------------------------------------------------------------------------------
COLLECT_LOADS = {
    "near_one": [(1.0, 1.0), (B.Bias(-15.0), B.Bias(-15.0)), (1.05, 1.05), (1.5, 1.0), (1.0, 2.0), (1.05, 1.0)],
    "thresholds": [(3.0, 3.0), (5.9999995, 5.9999995), (6.0, 6.0), (9.5, 9.5), (10.0, 1.0), (21.0, 2.1)],
    "trained": [(100.0, 100.0), (1000.0, 1000.0), (1000.0, 1.0), (1.0, 1000.0), (100.0, 10.0), (1000.0, 100.0)],
}
E_COL, T_COL = 37, 32
PATHS = {"per_step": "rollout=per_step", "k_rollout": "rollout_kernel=mfma", "k_rollout_v": "rollout_kernel=valu"}


def collect(load, options):
    """one rollout of the AC trainer at the load's parameters: (trainer, alpha, beta, actions, log-probs)"""
    L = Orc.layout_init(1, 17, 6, 256)
    p, al, be = B.head_params(L, np.random.default_rng(5), [t[0] for t in load], [t[1] for t in load])
    cfg = ppo_amd.ACPPOConfig(env_id="HalfCheetah-v5", num_envs=E_COL, num_steps=T_COL, num_minibatches=1,
                              update_epochs=1, total_timesteps=E_COL * T_COL * 4)
    tr = ppo_amd.Trainer(cfg, params=p, options=options)
    tr.rollout()
    tr.agent.sync()
    act = tr.agent.buffer(ppo_amd.BUF_ACTIONS, (T_COL, E_COL, 6)).numpy()
    lp = tr.agent.buffer(ppo_amd.BUF_LOGPROBS, (T_COL, E_COL)).numpy()
    return tr, al, be, act, lp


@pytest.mark.parametrize("name", list(COLLECT_LOADS))
def test_collection_paths(name):
    """One rollout of 37 envs x 32 steps on the synthetic cheetah through the per-step ppo_rollout_act
    launches, k_rollout and k_rollout_v (both with the deferred k_beta_logp: the public path defers for
    this agent): bitwise-equal action and log-prob buffers; every stored s in [1e-7 clamp, 1 - 2^-24] and
    every log-prob finite; the stored log-probs within the bound of beta_fp64 at the stored actions; per
    action dimension the first three sample moments within 5 sigma of the closed forms."""
    load = COLLECT_LOADS[name]
    runs = {k: collect(load, o) for k, o in PATHS.items()}
    try:
        _, al, be, act, lp = runs["per_step"]
        for k in ("k_rollout", "k_rollout_v"):
            np.testing.assert_array_equal(runs[k][3].view(np.uint32), act.view(np.uint32), err_msg=k + " actions")
            np.testing.assert_array_equal(runs[k][4].view(np.uint32), lp.view(np.uint32), err_msg=k + " logprobs")
        assert np.isfinite(lp).all()
        s = B.scale_action(act)
        assert s.max() <= B.S_MAX and (act >= B.LO).all() and (act < B.HI).all()
        a2 = act.reshape(-1, 6)
        ref = B.beta_fp64(*expand(al, be, a2.shape[0]), s.reshape(-1, 6))
        bd = B.row_bounds(ref, stored_action=a2)
        r = np.abs(lp.reshape(-1) - ref["lp"].numpy().sum(-1)) / bd["lp"]
        note("collection/" + name, "logp", r.max())
        assert (r <= 1).all(), r.max()
        for a in range(6):
            m = np.array(B.moment_check(s[:, :, a].ravel(), al[a], be[a]))
            note("sampler/" + name, "moments", m.max())
            assert (m < 1).all(), (load[a], m)
    finally:
        for r_ in runs.values():
            r_[0].close()


@pytest.mark.parametrize("name", list(COLLECT_LOADS))
def test_eval_sampled_action(name):
    """k_eval's sampled action: two sampled evaluation episodes give bitwise the returns of the per-step
    path (k_act3 + the env step), finite, at each parameter load."""
    load = COLLECT_LOADS[name]
    L = Orc.layout_init(1, 17, 6, 256)
    p, _, _ = B.head_params(L, np.random.default_rng(5), [t[0] for t in load], [t[1] for t in load])
    ag = make_agent(17, 6, 256)
    env = ppo_amd.SynthEnv(4, 17, 6)
    try:
        ag.load_params(p)
        fast = ag.evaluate(env, 2, ppo_amd.PPO_SAMPLE, eval_seed=3, num_eval_envs=2)
        assert ag.eval_info() == "eval=k_eval"
        slow = ag.evaluate(env, 2, ppo_amd.PPO_SAMPLE, eval_seed=3, num_eval_envs=2, per_step=True)
        assert np.isfinite(fast[0]).all()
        np.testing.assert_array_equal(fast[0].view(np.uint32), slow[0].view(np.uint32))
        np.testing.assert_array_equal(fast[1], slow[1])
    finally:
        ag.close(); env.close()


# ------------------------------------------------------------------------------------------------
# (c) update: every update copy
# ------------------------------------------------------------------------------------------------
UPDATE_COPIES = [((17, 6, 256), None, "k_upd/bx6"), ((17, 6, 256), "upd_mfma=16", "k_upd/f32"),
                 ((17, 6, 256), "upd_mfma=32", "k_upd32"), ((17, 6, 256), "upd_mfma=mix", "k_upd32/mix"),
                 ((17, 6, 256), "upd_kernel=fwdbwd", "k_fwdbwd"), ((11, 3, 256), None, "k_upd/bx6"),
                 ((17, 8, 256), None, "k_upd/bx6"), ((17, 8, 256), "upd_mfma=32", "k_upd32"),
                 ((17, 6, 64), "upd_kernel=fwdbwd", "k_fwdbwd")]


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("shape,opts,kernel", UPDATE_COPIES,
                         ids=["O%d_A%d_H%d-%s" % (s + (k.replace("/", "_"),)) for s, _, k in UPDATE_COPIES])
def test_update_head_gradients(shape, opts, kernel, setting):
    """One minibatch (M = 111, identity permutation, learning rate 0) per grid load: the head-bias
    gradients element by element against the fp64 restatement within their bound, the loss statistics
    within the bound of their row sums, clipfrac exactly. ent_coef = 0 isolates d logp, zero advantages
    with ent_coef = 1 isolate d ent.

    The head-weight gradients (row gradient times the actor's last hidden layer): element by element against
    the fp64 restatement with the rows' bounds carried through |h2|, and against the oracle at the per-tensor
    rel-L2 bar of test_gpu_update_headline.py (2e-3) wherever every row's log-prob bound is under 2e-4. Above
    that the flat bar cannot hold for any fp32 copy: a log-prob of magnitude 1.6e4 (s = 1 - 2^-24 under beta =
    1000) rounds by 1e-3 in fp32, the ratio and with it the row's whole gradient by 0.1 %, in the oracle as
    much as in a kernel. Measured against the oracle at the loads holding 100 and 1000: 2.0e-3 (k_upd, all
    forms), 2.3e-3 (A = 3), 2.6e-3 (k_fwdbwd); the element-wise bound covers those loads."""
    O_, A, H = shape
    M = E_UPD * T_UPD
    ent_coef = SETTINGS[setting]
    L = Orc.layout_init(1, O_, A, H)
    rng = np.random.default_rng(7 * O_ + A + H)
    o = "update_graph=0" + ("," + opts if opts else "")
    ag = make_agent(O_, A, H, E_UPD, T_UPD, ent=ent_coef, options=o)
    perm = DeviceArray.from_numpy(np.arange(M, dtype=np.int32))
    copy = "%s/A%d/H%d" % (kernel, A, H)
    try:
        assert ag.kernel_info().split()[0] in ("update=" + kernel, "update=" + kernel + "/hwg"), ag.kernel_info()
        for load in B.grid_loads(A):
            p, al, be = B.head_params(L, rng, [t[0] for t in load], [t[1] for t in load])
            act, ref, old, adv = B.update_case(al, be, M, rng)
            if setting == "ent":
                adv = np.zeros_like(adv)
            x = rng.standard_normal((M, O_)).astype(np.float32)
            ret, ov = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M).astype(np.float32)
            ag.load_params(p)
            fill_storage(ag, T_UPD, E_UPD, x, act, old, adv, ret, ov)
            st = ag.update(0.0, perms=perm, want_stats=True)
            g = ag.last_grad()
            u = B.update_fp64(ref, old, adv, CLIP, ent_coef, p[L.ab3:L.ab3 + A], p[L.bb3:L.bb3 + A])
            assert u["edge_margin"].min() > 1
            for h, off, q in (("a", L.ab3, "alpha"), ("b", L.bb3, "beta")):
                r = np.abs(g[off:off + A] - u["g" + h]) / u["g" + h + "_bound"]
                note(copy, "d" + setting + "/d" + q, r.max())
                assert (r <= 1).all(), (copy, setting, load, h, r, g[off:off + A], u["g" + h])
            og, _ = Orc.minibatch_grad(L, p, x, act, old, adv, ret, ov, Orc.LossCfg(CLIP, ent_coef, 0.5, 1, 0))
            h2 = B.actor_h2_fp64(L, p, x)
            for h, w in (("a", L.aW3), ("b", L.bW3)):
                gw, bw = B.head_weight_grad(u, h, h2)
                r = np.abs(g[w:w + A * H].reshape(A, H) - gw) / bw
                note(copy, "head weights", r.max())
                assert (r <= 1).all(), (copy, setting, load, h, r.max())
                if u["lp_bound"].max() < 2e-4 and np.linalg.norm(og[w:w + A * H]) > 1e-30:
                    rl2 = rel(g[w:w + A * H], og[w:w + A * H])
                    assert rl2 < 2e-3, (copy, setting, load, h, rl2)
            for k in ("pg_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac"):
                d = abs(st[k] - u["stats"][k])
                bound = u["stats_bound"][k] + 1e-6 * abs(u["stats"][k])
                if k != "clipfrac":
                    note(copy, "stat " + k, d / bound)
                assert d <= bound, (copy, setting, load, k, st[k], u["stats"][k], bound)
    finally:
        ag.close()


def test_a_above_8_is_out_of_reach_at_hidden_256():
    """k_upd's second Beta branch (A > 8: items in LDS) and k_act3's three-head-tile form exist for A in 17..20
    only, and ppo_create refuses those shapes for the LayerNorm-Beta agent: every context sizes k_fwdbwd's LDS
    for its 2 A head rows, which passes 160 KiB from A = 13 on. The refusal must leave no HIP error behind
    for the next call to find (it did: the following ppo_load_params of another context failed with
    "invalid argument")."""
    ag = make_agent(17, 6, 64)
    try:
        with pytest.raises(ppo_amd.PPOError, match="cannot set LDS size"):
            make_agent(17, 17, 256)
        L = Orc.layout_init(1, 17, 6, 64)
        p, _, _ = B.head_params(L, np.random.default_rng(0), [2.0] * 6, [3.0] * 6)
        ag.load_params(p)
        np.testing.assert_array_equal(ag.params(), p)
    finally:
        ag.close()


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_carla_update_head_gradients(setting):
    """k_carla_head_bwd: the dist_mu / dist_sigma bias gradients of one ppo_carla_update over 16 rows per
    grid load (learning rate 0, advantage normalisation off) against the fp64 restatement."""
    import carla_inputs as CI
    L = CI.layout()
    base = CI.params(L)
    n, ent_coef = 16, SETTINGS[setting]
    rng = np.random.default_rng(11)
    bev, meas, vmeas, _ = CI.inputs(n)
    ret, ov = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    fixed = [DeviceArray.from_numpy(bev, np.uint8)] + [DeviceArray.from_numpy(v) for v in (meas, vmeas)]
    ag = ppo_amd.CarlaAgent(max_batch=16, seed=7)
    try:
        for load in B.grid_loads(L.A):
            p, al, be = carla_head_params(L, base, load)
            act, ref, old, adv = B.update_case(al, be, n, rng)
            if setting == "ent":
                adv = np.zeros_like(adv)
            ag.load_params(p)
            d = fixed + [DeviceArray.from_numpy(np.ascontiguousarray(v, np.float32)) for v in (act, old, adv, ret, ov)]
            st = ag.update(*d, lr=0.0, clip_coef=CLIP, ent_coef=ent_coef, vf_coef=0.5, max_grad_norm=0.5,
                           adam_eps=1e-5, norm_adv=False)
            g = ag.last_grad()
            u = B.update_fp64(ref, old, adv, CLIP, ent_coef, p[L.mu_b:L.mu_b + L.A], p[L.sg_b:L.sg_b + L.A])
            assert u["edge_margin"].min() > 1
            for h, off, q in (("a", L.mu_b, "alpha"), ("b", L.sg_b, "beta")):
                r = np.abs(g[off:off + L.A] - u["g" + h]) / u["g" + h + "_bound"]
                note("k_carla_head_bwd", "d" + setting + "/d" + q, r.max())
                assert (r <= 1).all(), (setting, load, h, r, g[off:off + L.A], u["g" + h])
            for k in ("pg_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac"):
                bound = u["stats_bound"][k] + 1e-6 * abs(u["stats"][k])
                assert abs(st[k] - u["stats"][k]) <= bound, (setting, load, k, st[k], u["stats"][k], bound)
    finally:
        ag.close()


# ------------------------------------------------------------------------------------------------
# (d) first minibatch of epoch 0: collect path x update path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collect_opt", [None, "rollout=per_step"], ids=["persistent", "per_step"])
@pytest.mark.parametrize("update_opt", [None, "upd_kernel=fwdbwd"], ids=["k_upd", "k_fwdbwd"])
def test_first_minibatch_ratio_is_one(collect_opt, update_opt):
    """After a rollout at the trained load (concentrations 100 to 1000), GAE and one update with one
    minibatch and learning rate 0: old_logp came from the collection copy, new_logp from the update copy.
    In the reference both are the same LibTorch function and the statistics are zero up to the action round
    trip; here |old_approx_kl| and approx_kl are at most the mean over rows of twice the row's log-prob
    bound plus its round-trip term (the two copies' allowed errors), and no row is clipped."""
    opts = ",".join(o for o in (collect_opt, update_opt, "update_graph=0") if o)
    tr, al, be, act, lp = collect(COLLECT_LOADS["trained"], opts)
    try:
        tr.agent.compute_gae(tr.next_obs, tr.next_done)
        st = tr.agent.update(0.0, want_stats=True)
        a2 = act.reshape(-1, 6)
        ref = B.beta_fp64(*expand(al, be, a2.shape[0]), B.scale_action(a2))
        plain, stored = B.row_bounds(ref)["lp"], B.row_bounds(ref, stored_action=a2)["lp"]
        tol = (2 * plain + (stored - plain)).mean()
        note("first minibatch %s x %s" % (collect_opt or "persistent", update_opt or "k_upd"), "old_approx_kl",
             abs(st["old_approx_kl"]) / tol)
        assert abs(st["old_approx_kl"]) <= tol and 0 <= st["approx_kl"] + 1e-9 and st["approx_kl"] <= tol, (st, tol)
        assert st["clipfrac"] == 0.0
    finally:
        tr.close()


def test_zz_report():
    """prints the largest error / bound every copy measured (DESIGN section 4 records them)"""
    for (copy, q), v in sorted(WORST.items()):
        print("RATIO %-40s %-24s %.3f" % (copy, q, v))
