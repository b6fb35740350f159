"""GPU parity of the HIP hot path (through the C-ABI) against the reference-arithmetic golden
vectors (tests/golden) and the CPU oracle (oracle/ppo_oracle.c) on the same seeded inputs.

Tolerances (fp32 throughout, MFMA f32 = exact fp32 FMA chains, oracle accumulates in double):
  forward values / log-probs / entropies   rtol 2e-5 .. 1e-4 (sums of O(10) terms)
  raw gradients                            relative L2 error < 2e-4 overall, < 2e-3 per tensor
  parameters after Adam                     atol 2e-6 per step (lr = 2.5e-4 .. 3e-4)
  GAE, env dynamics, permutations           bit-exact
"""
import os

import numpy as np
import pytest

import oracle_lib as O
from golden_io import load_case

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def make_agent(kind, O_, A, H, E, T=1, MB=1, EP=1, clip=0.2, ent=0.01, vf=0.5, max_grad_norm=0.5, adam_eps=1e-5,
               seed=1, norm_adv=1, clip_vloss=1, options=None):
    hc = ppo_amd.HipConfig(kind, O_, A, H, E, T, MB, EP, 0.99, 0.95, clip, ent, vf, max_grad_norm, adam_eps,
                           norm_adv, clip_vloss, seed, 0, 1)
    return ppo_amd.Agent(hc, options=options)


def fill_storage(ag, T, E, obs, act, logp, adv, ret, val):
    ag.buffer(ppo_amd.BUF_OBS, (T, E, ag.O)).upload(obs.reshape(T, E, ag.O))
    ag.buffer(ppo_amd.BUF_ACTIONS, (T, E, ag.A)).upload(act.reshape(T, E, ag.A))
    ag.buffer(ppo_amd.BUF_LOGPROBS, (T, E)).upload(logp.reshape(T, E))
    ag.buffer(ppo_amd.BUF_ADVANTAGES, (T, E)).upload(adv.reshape(T, E))
    ag.buffer(ppo_amd.BUF_RETURNS, (T, E)).upload(ret.reshape(T, E))
    ag.buffer(ppo_amd.BUF_VALUES, (T, E)).upload(val.reshape(T, E))


def random_params(L, rng, scale=1.0):
    p = np.zeros(L.P, np.float32)
    for t in range(L.ntensors):
        o, n = L.t_off[t], L.t_len[t]
        p[o:o + n] = rng.standard_normal(n).astype(np.float32) * 0.1
    if L.kind == 1:
        p[L.hi], p[L.lo] = 1.0, -1.0
        p[L.ostd:L.ostd + L.O] = rng.uniform(0.8, 1.5, L.O)
        for tr in (L.critic, L.actor):
            p[tr[2]:tr[2] + L.H] = rng.uniform(0.8, 1.2, L.H)  # LN gamma
            p[tr[6]:tr[6] + L.H] = rng.uniform(0.8, 1.2, L.H)
    for tr in (L.critic, L.actor):
        p[tr[0]:tr[0] + L.H * L.O] = rng.standard_normal(L.H * L.O) / np.sqrt(L.O)
        p[tr[4]:tr[4] + L.H * L.H] = rng.standard_normal(L.H * L.H) / np.sqrt(L.H)
    return (p * 1.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# act (Agent::get_action_and_value) vs golden and oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,kind", [("ppo_act", 0), ("ac_act", 1)])
def test_act_given_action_vs_golden(case, kind):
    meta, d = load_case(case)
    n = d["x"].shape[0]
    ag = make_agent(kind, meta["O"], meta["A"], meta["H"], n)
    ag.load_params(d["params"])
    np.testing.assert_array_equal(ag.params(), d["params"])  # pack/unpack round trip
    x = DeviceArray.from_numpy(d["x"])
    a = DeviceArray.from_numpy(d["action"])
    act, lp, ent, v = ag.get_action_and_value(x, ppo_amd.PPO_GIVEN, a)
    np.testing.assert_allclose(lp.numpy(), d["logprob"], rtol=2e-5, atol=5e-5)
    np.testing.assert_allclose(ent.numpy(), d["entropy"], rtol=2e-5, atol=5e-5)
    np.testing.assert_allclose(v.numpy(), d["value"], rtol=2e-5, atol=2e-5)
    if kind == 1:
        np.testing.assert_allclose(act.numpy(), d["action_roundtrip"], rtol=0, atol=2e-7)
        am, lpm, _, _ = ag.get_action_and_value(x, ppo_amd.PPO_MEAN)
        np.testing.assert_allclose(am.numpy(), d["mean_action"], rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(lpm.numpy(), d["mean_logprob"], rtol=2e-5, atol=5e-5)
    else:
        am, _, _, _ = ag.get_action_and_value(x, ppo_amd.PPO_MEAN)
        np.testing.assert_allclose(am.numpy(), d["mean"], rtol=1e-5, atol=2e-6)


# The update=off cases: the LayerNorm-Beta agent at hidden 256 with 2 A = 34 to 40 head rows, live head weights
# in all three head tiles of k_act3 (acting-only contexts; one that updates is refused from A = 13 on): <24, 3>
# at O = 376, at O = 373 (a ragged last k-block of layer 1) and at O = OP = 384 with the widest A, <2, 3> at
# O = 17. n A >= 3 400 leaves the sampled-action cap room for three accept flips (the cases before: at least
# one, at 1 600 items); every n ends on a ragged 16-row workgroup.
ACT_ORACLE_CASES = [(1, 17, 6, 256, 1000, None), (0, 17, 6, 64, 777, None), (0, 376, 17, 64, 300, None),
                    (1, 105, 8, 256, 200, None), (1, 376, 17, 256, 200, "update=off"), (1, 373, 17, 256, 200, "update=off"),
                    (1, 384, 20, 256, 170, "update=off"), (1, 17, 17, 256, 200, "update=off")]


@pytest.mark.parametrize("kind,O_,A,H,n,options", ACT_ORACLE_CASES,
                         ids=["-".join(str(v) for v in c[:5]) + ("-" + c[5].replace("=", "_") if c[5] else "")
                              for c in ACT_ORACLE_CASES])
def test_act_vs_oracle_given_mean_sample(kind, O_, A, H, n, options):
    rng = np.random.default_rng(7)
    ag = make_agent(kind, O_, A, H, n, options=options)
    L = O.layout_init(kind, O_, A, H)
    p = random_params(L, rng)
    ag.load_params(p)
    x = rng.standard_normal((n, O_)).astype(np.float32)
    act = rng.uniform(-0.95, 0.95, (n, A)).astype(np.float32)
    if kind == 0:
        act = rng.standard_normal((n, A)).astype(np.float32)
    xd, ad = DeviceArray.from_numpy(x), DeviceArray.from_numpy(act)
    # given action
    _, lp, ent, v = ag.get_action_and_value(xd, ppo_amd.PPO_GIVEN, ad)
    _, olp, oent, ov = O.get_action_and_value(L, p, x, 1, act)
    np.testing.assert_allclose(v.numpy(), ov, rtol=1e-4, atol=5e-5)
    np.testing.assert_allclose(lp.numpy(), olp, rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose(ent.numpy(), oent, rtol=1e-4, atol=2e-4)
    # deterministic mean action
    am, lpm, _, _ = ag.get_action_and_value(xd, ppo_amd.PPO_MEAN)
    oam, olpm, _, _ = O.get_action_and_value(L, p, x, 2)
    np.testing.assert_allclose(am.numpy(), oam, rtol=1e-4, atol=2e-5)
    # sampled actions: same Philox counters; differences only from libm vs ocml ulps
    sa, slp, _, _ = ag.get_action_and_value(xd, ppo_amd.PPO_SAMPLE, env_base=5, step_id=123)
    osa, oslp, _, _ = O.get_action_and_value(L, p, x, 0, seed=1, rank=0, env_base=5, step_id=123)
    sa = sa.numpy()
    close = np.isclose(sa, osa, rtol=1e-4, atol=5e-5)
    assert close.mean() > 0.999, close.mean()   # a rare Marsaglia-Tsang accept flip is allowed
    rows = close.all(axis=1)
    np.testing.assert_allclose(slp.numpy()[rows], oslp[rows], rtol=1e-3, atol=1e-3)
    if kind == 1:
        assert np.all(sa > -1.0) and np.all(sa < 1.0)


def test_beta_sampler_moments():
    """Marsaglia-Tsang Beta samples have the right mean/variance (replaces at::_sample_dirichlet)."""
    n, O_, A, H = 8192, 17, 6, 64
    ag = make_agent(1, O_, A, H, n)
    L = O.layout_init(1, O_, A, H)
    p = np.zeros(L.P, np.float32)
    p[L.hi], p[L.lo] = 1.0, -1.0
    p[L.ostd:L.ostd + O_] = 1.0
    for tr in (L.critic, L.actor):
        p[tr[2]:tr[2] + H] = 1.0; p[tr[6]:tr[6] + H] = 1.0
    # heads: constant pre-activations -> alpha = softplus(1.5)+1, beta = softplus(-0.5)+1
    p[L.ab3:L.ab3 + A] = 1.5
    p[L.bb3:L.bb3 + A] = -0.5
    ag.load_params(p)
    x = DeviceArray.from_numpy(np.zeros((n, O_), np.float32))
    a, _, _, _ = ag.get_action_and_value(x, ppo_amd.PPO_SAMPLE, step_id=99)
    s = (a.numpy() + 1.0) / 2.0
    al = np.log1p(np.exp(1.5)) + 1; be = np.log1p(np.exp(-0.5)) + 1
    mean = al / (al + be); var = al * be / ((al + be) ** 2 * (al + be + 1))
    assert abs(s.mean() - mean) < 4 * np.sqrt(var / s.size)
    assert abs(s.var() - var) / var < 0.02


# ------------------------------------------------------------------------------------------------
# GAE
# ------------------------------------------------------------------------------------------------
def test_gae_bit_exact_vs_golden():
    meta, d = load_case("gae")
    T, E = d["rewards"].shape
    ag = make_agent(0, 17, 6, 64, E, T=T)
    ag.buffer(ppo_amd.BUF_REWARDS, (T, E)).upload(d["rewards"])
    ag.buffer(ppo_amd.BUF_VALUES, (T, E)).upload(d["values"])
    ag.buffer(ppo_amd.BUF_DONES, (T, E)).upload(d["dones"])
    ag.gae_from_values(DeviceArray.from_numpy(d["next_value"]), DeviceArray.from_numpy(d["next_done"]))
    np.testing.assert_array_equal(ag.buffer(ppo_amd.BUF_ADVANTAGES, (T, E)).numpy(), d["advantages"])
    np.testing.assert_array_equal(ag.buffer(ppo_amd.BUF_RETURNS, (T, E)).numpy(), d["returns"])


def test_gae_full_size_bit_exact_vs_oracle():
    T, E = 128, 4096
    rng = np.random.default_rng(3)
    r = rng.standard_normal((T, E)).astype(np.float32)
    v = rng.standard_normal((T, E)).astype(np.float32)
    dn = (rng.random((T, E)) < 0.001).astype(np.float32)
    dn[0] = 1.0
    nv = rng.standard_normal(E).astype(np.float32)
    nd = (rng.random(E) < 0.5).astype(np.float32)
    ag = make_agent(1, 17, 6, 256, E, T=T, MB=4, EP=1)
    ag.buffer(ppo_amd.BUF_REWARDS, (T, E)).upload(r)
    ag.buffer(ppo_amd.BUF_VALUES, (T, E)).upload(v)
    ag.buffer(ppo_amd.BUF_DONES, (T, E)).upload(dn)
    ag.gae_from_values(DeviceArray.from_numpy(nv), DeviceArray.from_numpy(nd))
    oa, orr = O.gae(r, v, dn, nv, nd, 0.99, 0.95)
    np.testing.assert_array_equal(ag.buffer(ppo_amd.BUF_ADVANTAGES, (T, E)).numpy(), oa)
    np.testing.assert_array_equal(ag.buffer(ppo_amd.BUF_RETURNS, (T, E)).numpy(), orr)


@pytest.mark.parametrize("T,E", [(2048, 1024), (128, 4096), (37, 1000), (5, 70)])
def test_gae_scan_matches_serial(T, E):
    """gae=scan (k_gae_scan: 16 segments of the steps per 64-env workgroup; each segment's affine
    maps composed from the end, then the serial recurrence from the composed incoming value) against
    the bit-exact serial k_gae on the same buffers: cfg2's T = 2 048 / E = 1 024, the metric's
    T = 128 / E = 4 096, ragged E and T shorter than the 16 segments. The composed incoming values round
    differently: advantages within rtol 1e-5 / atol 1e-5 (measured max |d| is printed), returns too."""
    rng = np.random.default_rng(19)
    r = rng.standard_normal((T, E)).astype(np.float32)
    v = (rng.standard_normal((T, E)) * 3.0).astype(np.float32)
    dn = (rng.random((T, E)) < 0.002).astype(np.float32)
    nv = rng.standard_normal(E).astype(np.float32)
    nd = (rng.random(E) < 0.5).astype(np.float32)
    out = []
    for opt in ("gae=serial", "gae=scan"):
        ag = make_agent(0, 17, 6, 64, E, T=T, options=opt)
        ag.buffer(ppo_amd.BUF_REWARDS, (T, E)).upload(r)
        ag.buffer(ppo_amd.BUF_VALUES, (T, E)).upload(v)
        ag.buffer(ppo_amd.BUF_DONES, (T, E)).upload(dn)
        ag.gae_from_values(DeviceArray.from_numpy(nv), DeviceArray.from_numpy(nd))
        out.append((ag.buffer(ppo_amd.BUF_ADVANTAGES, (T, E)).numpy(), ag.buffer(ppo_amd.BUF_RETURNS, (T, E)).numpy()))
        ag.close()
    (a0, r0), (a1, r1) = out
    print(f"\nT={T} E={E}: max |adv scan - serial| {np.abs(a1 - a0).max():.2e} (max |adv| {np.abs(a0).max():.1f})")
    np.testing.assert_allclose(a1, a0, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(r1, r0, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------
# minibatch update (loss, backward, clip_grad_norm_, Adam) vs golden
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,kind", [("ppo_update", 0), ("ac_update", 1)])
def test_update_vs_golden(case, kind):
    meta, d = load_case(case)
    M = meta["M"]
    ag = make_agent(kind, meta["O"], meta["A"], meta["H"], M, T=1, MB=1, EP=1, clip=meta["clip_coef"],
                    ent=meta["ent_coef"], vf=meta["vf_coef"], max_grad_norm=meta["max_grad_norm"],
                    adam_eps=meta["adam_eps"])
    ag.load_params(d["params"])
    fill_storage(ag, 1, M, d["x"], d["action"], d["old_logp"], d["adv"], d["ret"], d["old_v"])
    perm = DeviceArray.from_numpy(np.arange(M, dtype=np.int32))
    st = ag.update(meta["lr"], perms=perm)
    g = ag.last_grad()
    assert rel(g, d["grad_raw"]) < 2e-4
    L = ag.layout
    for t in range(L.ntensors):
        o, n = L.t_off[t], L.t_len[t]
        if L.t_grad[t]:
            assert rel(g[o:o + n], d["grad_raw"][o:o + n]) < 2e-3, t
    gs = d["stats"]
    np.testing.assert_allclose([st["pg_loss"], st["v_loss"], st["entropy"], st["old_approx_kl"], st["approx_kl"],
                                st["clipfrac"]], gs[:6], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(st["grad_norm"], d["total_norm"][0], rtol=2e-4)
    np.testing.assert_allclose(ag.params(), d["params_step1"], rtol=0, atol=2e-6)
    ag.update(meta["lr"], perms=perm)
    ag.update(meta["lr"], perms=perm)
    np.testing.assert_allclose(ag.params(), d["params_step3"], rtol=0, atol=6e-6)


@pytest.mark.parametrize("kind,O_,A,H,E,T,MB", [(1, 17, 6, 256, 256, 4, 1), (1, 17, 6, 256, 200, 3, 2),
                                               (0, 376, 17, 64, 96, 4, 2), (1, 105, 8, 256, 64, 4, 1)])
def test_minibatch_grad_vs_oracle(kind, O_, A, H, E, T, MB):
    rng = np.random.default_rng(11)
    L = O.layout_init(kind, O_, A, H)
    p = random_params(L, rng)
    B = T * E
    x = rng.standard_normal((B, O_)).astype(np.float32)
    act = (rng.uniform(-0.95, 0.95, (B, A)) if kind else rng.standard_normal((B, A))).astype(np.float32)
    _, lp0, _, v0 = O.get_action_and_value(L, p, x, 1, act)
    olp = (lp0 + rng.standard_normal(B) * 0.1).astype(np.float32)
    ov = (v0 + rng.standard_normal(B) * 0.1).astype(np.float32)
    adv = rng.standard_normal(B).astype(np.float32)
    ret = rng.standard_normal(B).astype(np.float32)
    clip = 0.1 if kind else 0.2
    ag = make_agent(kind, O_, A, H, E, T=T, MB=MB, EP=1, clip=clip)
    ag.load_params(p)
    fill_storage(ag, T, E, x, act, olp, adv, ret, ov)
    perm = rng.permutation(B).astype(np.int32)
    ag.update(2.5e-4, perms=DeviceArray.from_numpy(perm))
    g = ag.last_grad()
    M = B // MB
    sl = perm[(MB - 1) * M:]  # last minibatch
    cfg = O.LossCfg(clip, 0.01, 0.5, 1, 1)
    if MB == 1:
        og, _ = O.minibatch_grad(L, p, x[sl], act[sl], olp[sl], adv[sl], ret[sl], ov[sl], cfg)
        assert rel(g, og) < 5e-4
        for t in range(L.ntensors):
            o, n = L.t_off[t], L.t_len[t]
            if L.t_grad[t]:
                assert rel(g[o:o + n], og[o:o + n]) < 5e-3, (t, rel(g[o:o + n], og[o:o + n]))
    # whole update (all minibatches, clip + Adam) vs the oracle's update loop
    ag2 = make_agent(kind, O_, A, H, E, T=T, MB=MB, EP=1, clip=clip)
    ag2.load_params(p)
    fill_storage(ag2, T, E, x, act, olp, adv, ret, ov)
    ag2.update(2.5e-4, perms=DeviceArray.from_numpy(perm))
    op, _, _, _, _ = O.update(L, p, np.zeros(L.P), np.zeros(L.P), 0, x, act, olp, adv, ret, ov, 1, MB, 2.5e-4, 0.5,
                              1e-5, cfg, perms=perm.astype(np.int64)[None, :])
    np.testing.assert_allclose(ag2.params(), op, rtol=0, atol=2e-6 * MB)


def test_permutation_matches_oracle_and_is_a_permutation():
    """Feistel minibatch permutation (replaces torch::randperm) — bit-exact with the oracle."""
    E, T, MB, EP = 64, 8, 2, 2
    rng = np.random.default_rng(5)
    L = O.layout_init(0, 17, 6, 64)
    p = random_params(L, rng)
    B = E * T
    x = rng.standard_normal((B, 17)).astype(np.float32)
    act = rng.standard_normal((B, 6)).astype(np.float32)
    _, lp0, _, v0 = O.get_action_and_value(L, p, x, 1, act)
    adv = rng.standard_normal(B).astype(np.float32)
    ret = rng.standard_normal(B).astype(np.float32)
    ag = make_agent(0, 17, 6, 64, E, T=T, MB=MB, EP=EP)
    ag.load_params(p)
    fill_storage(ag, T, E, x, act, lp0, adv, ret, v0)
    ag.set_iteration(3)
    ag.update(3e-4)
    cfg = O.LossCfg(0.2, 0.01, 0.5, 1, 1)
    op, _, _, _, _ = O.update(L, p, np.zeros(L.P), np.zeros(L.P), 0, x, act, lp0, adv, ret, v0, EP, MB, 3e-4, 0.5,
                              1e-5, cfg, seed=1, rank=0, epoch_counter0=3 * EP)
    np.testing.assert_allclose(ag.params(), op, rtol=0, atol=1e-5)
    for B_ in (1, 7, 64, 1000, 524288):
        pr = O.perm(B_, 1, 0, 5)
        assert np.array_equal(np.sort(pr), np.arange(B_))


# ------------------------------------------------------------------------------------------------
# synthetic device env vs oracle env (bit-exact) and a full small iteration vs the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O_,A", [(17, 6), (105, 8), (376, 17)])
def test_synth_env_bit_exact_vs_oracle(O_, A):
    """k_synth_step (O <= 32) and k_synth_step_wide (Ant / Humanoid widths) vs the oracle env."""
    E = 300
    env = ppo_amd.SynthEnv(E, O_, A)
    oenv = O.SynthEnv(E, O_, A)
    obs = DeviceArray((E, O_)); done = DeviceArray(E); rew = DeviceArray(E)
    env.reset(7, obs, done)
    o_obs = oenv.reset(7)
    np.testing.assert_array_equal(obs.numpy(), o_obs)
    rng = np.random.default_rng(0)
    for t in range(1005):
        a = rng.uniform(-1.3, 1.3, (E, A)).astype(np.float32)
        env.step(DeviceArray.from_numpy(a), obs, rew, done)
        o_obs, o_r, o_te, o_tr, _, _ = oenv.step(a)
        if t % 97 == 0 or t >= 998:
            np.testing.assert_array_equal(obs.numpy(), o_obs)
            np.testing.assert_array_equal(rew.numpy(), o_r)
            np.testing.assert_array_equal(done.numpy(), np.maximum(o_te, o_tr))
    sr, sl, n = env.episode_stats()
    assert n == E and abs(sl - 1000 * E) < 1e-3


@pytest.mark.parametrize("kind", [0, 1])
def test_full_iteration_vs_oracle(kind):
    """rollout (act + env) -> GAE -> update for E=64, T=16, MB=2, EP=2, against the oracle doing
    the same with the same Philox counters and Feistel permutations."""
    E, T, MB, EP = 64, 16, 2, 2
    O_, A, H = 17, 6, (64 if kind == 0 else 256)
    rng = np.random.default_rng(21)
    L = O.layout_init(kind, O_, A, H)
    p = random_params(L, rng)
    if kind == 0:
        p[L.logstd:L.logstd + A] = -0.5
    clip = 0.2 if kind == 0 else 0.1
    cfg = ppo_amd.PPOConfig(num_envs=E, num_steps=T, num_minibatches=MB, update_epochs=EP, env_id="HalfCheetah-v5",
                            net_kind=kind, hidden=H, clip_coef=clip, ent_coef=0.01, total_timesteps=E * T * 4)
    tr = ppo_amd.Trainer(cfg, params=p)
    tr.iterate()
    gpu_p = tr.agent.params()
    gpu_obs = tr.agent.buffer(ppo_amd.BUF_OBS, (T, E, O_)).numpy()
    gpu_adv = tr.agent.buffer(ppo_amd.BUF_ADVANTAGES, (T, E)).numpy()
    gb = {k: tr.agent.buffer(b, (T, E)).numpy() for k, b in (("logp", ppo_amd.BUF_LOGPROBS),
                                                              ("ret", ppo_amd.BUF_RETURNS),
                                                              ("val", ppo_amd.BUF_VALUES))}
    gpu_act = tr.agent.buffer(ppo_amd.BUF_ACTIONS, (T, E, A)).numpy()
    # oracle replay (the PPO trainer's envs carry the wrapper chain of ppo:41-49, the AC trainer's not)
    oenv = O.SynthEnv(E, O_, A, wrappers=(kind == 0), gamma=cfg.gamma)
    nobs = oenv.reset(cfg.seed)
    ndone = np.zeros(E, np.float32)
    bo = np.zeros((T, E, O_), np.float32); ba = np.zeros((T, E, A), np.float32)
    bl = np.zeros((T, E), np.float32); br = np.zeros((T, E), np.float32)
    bd = np.zeros((T, E), np.float32); bv = np.zeros((T, E), np.float32)
    for t in range(T):
        bo[t] = nobs; bd[t] = ndone
        a, lp, _, v = O.get_action_and_value(L, p, nobs, 0, seed=cfg.seed, rank=0, env_base=0, step_id=t)
        ba[t] = a; bl[t] = lp; bv[t] = v
        nobs, r, te, trn, _, _ = oenv.step(a)
        br[t] = r
        ndone = np.maximum(te, trn)
    _, _, _, nv = O.get_action_and_value(L, p, nobs, 2)
    adv, ret = O.gae(br, bv, bd, nv, ndone, 0.99, 0.95)
    np.testing.assert_allclose(gpu_obs, bo, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(gpu_adv, adv, rtol=1e-3, atol=1e-3)
    lcfg = O.LossCfg(clip, 0.01, 0.5, 1, 1)
    lr = float(np.float32(1.0) * np.float32(cfg.learning_rate))
    np.testing.assert_allclose(gpu_act, ba, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(gb["logp"], bl, rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(gb["ret"], ret, rtol=1e-3, atol=1e-3)
    op, _, _, _, _ = O.update(L, p, np.zeros(L.P), np.zeros(L.P), 0, gpu_obs.reshape(-1, O_), gpu_act.reshape(-1, A),
                              gb["logp"].reshape(-1), gpu_adv.reshape(-1), gb["ret"].reshape(-1),
                              gb["val"].reshape(-1), EP, MB, lr, 0.5, 1e-5, lcfg, seed=cfg.seed, rank=0,
                              epoch_counter0=0)
    # Adam's first steps move a parameter by ~ lr g / (|g| + eps): an element whose minibatch gradient
    # is a near-cancelling sum (|g| ~ eps) turns an fp32 rounding difference of that sum into an
    # lr-sized step difference (test_gpu_update_headline's per-element bound). Such elements must
    # stay a tiny minority (measured: 0 with fp32 MFMAs, 2 of 146 225 with k_upd's split-bf16 GEMMs,
    # 3.7e-5 = 0.15 lr), every other parameter within 2e-5.
    d = np.abs(gpu_p.astype(np.float64) - op)
    assert (d > 2e-5).mean() < 1e-4 and d.max() < 0.5 * lr, ((d > 2e-5).sum(), d.max())


@pytest.mark.parametrize("E,EP,opts", [(4096, 2, None), (512, 4, None),
                                        (512, 4, "upd_mfma=16,dw_mfma=f32,values_mfma=f32")])
def test_trainer_iteration_vs_oracle_at_metric_size(E, EP, opts):
    """One whole AC trainer iteration at the metric shape (E = 4 096, T = 128, 4 minibatches of
    131 072 rows; 2 of the 4 epochs to bound the oracle's time) and at the N = 8 shard (E = 512:
    k_rollout_v, 16 minibatches of 16 384 rows), with the split-bf16 defaults, against the oracle:
    - rollout, teacher-forced per step: the oracle's act (same Philox counters) on the GPU's stored
      observations of two 64-env blocks at every step, and the oracle env stepped with the GPU's
      actions for all envs (its observations and rewards vs the GPU's);
    - GAE on the GPU's rewards / values / dones with the oracle's bootstrap;
    - the update: the oracle's minibatch chain (Feistel permutations, per-minibatch advantage
      normalisation, clip_grad_norm_, Adam; ac:786-888) from the GPU's rollout buffers, row sums
      on a thread pool (minibatch_grad_parallel), against the GPU's parameters after the iteration.
    Bars: acts / logp / values within the E = 64 full-iteration test's (a Marsaglia-Tsang acceptance
    flipped by an fp32 rounding may change single samples: at most 1e-4 of them); parameters: the
    median within 2e-6, 99 % within 5e-5, at most 3 % beyond 2e-5, none beyond lr. The tail is the
    actor's near-zero gradients: with |g| ~ 1e-6 (Adam's v ~ 1e-12, below eps = 1e-5) the fp32 sums
    of a minibatch keep a relative rounding error that the fp64 oracle does not, and each Adam step
    turns it into a fraction of lr. Measured (MI355X): E = 4 096, 2 epochs (8 steps): max 7.0e-6,
    none beyond 2e-5; E = 512, 4 epochs (16 steps): max 1.26e-4 (0.5 lr), 1.4 % beyond 2e-5 with
    the split-bf16 defaults and 1.7 % with every GEMM on fp32 MFMAs (same max): the fp32 arithmetic,
    not the split products; 1 epoch at E = 512: max 7.3e-6."""
    T, MB, O_, A, H = 128, 4, 17, 6, 256
    cfg = ppo_amd.ACPPOConfig(env_id="HalfCheetah-v5", num_envs=E, num_steps=T, num_minibatches=MB, update_epochs=EP,
                              total_timesteps=E * T * 4)
    tr = ppo_amd.Trainer(cfg, options=opts)
    try:
        assert tr.agent.kernel_info().startswith("update=k_upd/bx6" if opts is None else "update=k_upd/f32")
        p0 = tr.agent.params().copy()
        tr.iterate()
        tr.agent.sync()
        gpu_p = tr.agent.params()
        g = {k: tr.agent.buffer(b, (T, E)).numpy() for k, b in (("logp", ppo_amd.BUF_LOGPROBS), ("rew", ppo_amd.BUF_REWARDS),
                                                               ("done", ppo_amd.BUF_DONES), ("val", ppo_amd.BUF_VALUES),
                                                               ("adv", ppo_amd.BUF_ADVANTAGES), ("ret", ppo_amd.BUF_RETURNS))}
        gobs = tr.agent.buffer(ppo_amd.BUF_OBS, (T, E, O_)).numpy()
        gact = tr.agent.buffer(ppo_amd.BUF_ACTIONS, (T, E, A)).numpy()
    finally:
        tr.close()
    L = O.layout_init(1, O_, A, H)
    # rollout: oracle env driven by the GPU's actions; oracle acts on the GPU's observations
    oenv = O.SynthEnv(E, O_, A, wrappers=False, gamma=cfg.gamma)
    nobs = oenv.reset(cfg.seed)
    np.testing.assert_allclose(gobs[0], nobs, rtol=1e-5, atol=1e-6)
    blocks = [(0, 64), (E // 2, E // 2 + 64)]
    bad = tot = 0
    orew = np.zeros((T, E), np.float32)
    for t in range(T):
        if t > 0:
            np.testing.assert_allclose(gobs[t], nobs, rtol=1e-4, atol=1e-5)
        for e0, e1 in blocks:
            a, lp, _, v = O.get_action_and_value(L, p0, gobs[t, e0:e1], 0, seed=cfg.seed, rank=0, env_base=e0, step_id=t)
            close = np.isclose(gact[t, e0:e1], a, rtol=1e-4, atol=1e-4).all(axis=1)
            close &= np.isclose(g["logp"][t, e0:e1], lp, rtol=1e-4, atol=1e-3)
            close &= np.isclose(g["val"][t, e0:e1], v, rtol=2e-5, atol=2e-5)
            bad += int((~close).sum()); tot += close.size
        nobs, r, te, trn, _, _ = oenv.step(gact[t])
        orew[t] = r
        ndone = np.maximum(te, trn)
    assert bad <= max(1, 1e-4 * tot), (bad, tot)
    np.testing.assert_allclose(g["rew"], orew, rtol=1e-5, atol=1e-6)
    _, _, _, nv = O.get_action_and_value(L, p0, nobs, 2)
    adv, ret = O.gae(g["rew"], g["val"], g["done"], nv, ndone, cfg.gamma, cfg.gae_lambda)
    np.testing.assert_allclose(g["adv"], adv, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(g["ret"], ret, rtol=1e-3, atol=1e-3)
    # update: the oracle's minibatch chain (orc_update's loop) from the GPU's buffers
    B = T * E
    Mb = B // MB
    bo, ba = gobs.reshape(B, O_), gact.reshape(B, A)
    bl, bad_, br, bv = (g[k].reshape(B) for k in ("logp", "adv", "ret", "val"))
    lcfg = O.LossCfg(cfg.clip_coef, cfg.ent_coef, cfg.vf_coef, int(cfg.clip_vloss), int(cfg.norm_adv))
    lr = float(np.float32(1.0) * np.float32(cfg.learning_rate))
    p = p0.astype(np.float32).copy()
    m = np.zeros(L.P, np.float32); v = np.zeros(L.P, np.float32)
    step = 0
    for e in range(EP):
        perm = O.perm(B, cfg.seed, 0, e)
        for s0 in range(0, B, Mb):
            j = perm[s0:s0 + Mb]
            grad, _ = O.minibatch_grad_parallel(L, p, bo[j], ba[j], bl[j], bad_[j], br[j], bv[j], lcfg)
            grad, _ = O.clip_grad_norm(L, grad, cfg.max_grad_norm)
            step += 1
            p, m, v = O.adam_step(L, p, grad, m, v, step, lr, cfg.adam_eps)
    d = np.abs(gpu_p.astype(np.float64) - p)
    print(f"\nE={E} EP={EP} {opts}: params max |d| {d.max():.2e} ({d.max() / lr:.3f} lr), > 2e-5: {(d > 2e-5).sum()} of {d.size}; "
          f"rollout act mismatches {bad} of {tot}")
    print("|d| quantiles 0.5 / 0.9 / 0.99 / 0.999:", np.quantile(d, [0.5, 0.9, 0.99, 0.999]))
    if os.environ.get("PPO_TEST_DIAG"):
        offs = [(int(L.t_off[i]), int(L.t_len[i])) for i in range(L.ntensors)]
        for k in np.argsort(-d)[:12]:
            ti = [i for i, (o, n) in enumerate(offs) if o <= k < o + n]
            print(f"  elem {k} tensor {ti} p0 {p0[k]:+.6e} gpu {gpu_p[k]:+.6e} oracle {p[k]:+.6e} m {m[k]:+.3e} v {v[k]:.3e}")
        big = d > 2e-5
        for i, (o, n) in enumerate(offs):
            nb = int(big[o:o + n].sum())
            if nb:
                print(f"  tensor {i} off {o} len {n}: {nb} elements > 2e-5, max {d[o:o + n].max():.2e}")
    q50, q99 = np.quantile(d, [0.5, 0.99])
    assert q50 < 2e-6 and q99 < 5e-5 and (d > 2e-5).mean() < 0.03 and d.max() < lr, (q50, q99, (d > 2e-5).sum(), d.max())


# ------------------------------------------------------------------------------------------------
# metric configuration (AC-PPO HalfCheetah, E=4096, T=128, MB=4, EP=4): size-independent checks
# ------------------------------------------------------------------------------------------------
def test_metric_config_iteration_properties_and_determinism():
    cfg = ppo_amd.ACPPOConfig(num_envs=4096, env_id="HalfCheetah-v5", total_timesteps=4096 * 128 * 10)
    res = []
    for rep in range(2):
        tr = ppo_amd.Trainer(cfg)
        st = tr.iterate(want_stats=True)
        res.append((tr.agent.params(), st))
        tr.close()
    (p0, s0), (p1, s1) = res
    assert np.isfinite(p0).all()
    np.testing.assert_array_equal(p0, p1)          # bitwise deterministic (no atomics anywhere)
    assert s0 == s1
    assert s0["minibatches"] == 16
    for k in ("pg_loss", "v_loss", "entropy", "approx_kl", "clipfrac", "grad_norm"):
        assert np.isfinite(s0[k]), k
    assert 0.0 <= s0["clipfrac"] <= 1.0
    assert s0["grad_norm"] > 0


@pytest.mark.parametrize("kind,O_,A,H", [(1, 17, 6, 256), (0, 17, 6, 256), (0, 17, 6, 64), (0, 376, 17, 64),
                                         (0, 11, 3, 64)])
def test_update_kernels_agree(kind, O_, A, H):
    """The feature-split k_upd (H = 256) / the two-trunk k_upd2 (H = 64) and the wave-per-16-rows
    k_fwdbwd compute the same minibatch gradient (different summation orders only) at a size where
    every workgroup loops several times (M = 12 792 rows, ragged last tile)."""
    rng = np.random.default_rng(5)
    L = O.layout_init(kind, O_, A, H)
    p = random_params(L, rng)
    if kind == 0:
        p[L.logstd:L.logstd + A] = -0.5
    E, T = 1599, 8
    B = T * E
    x = rng.standard_normal((B, O_)).astype(np.float32)
    act = (rng.uniform(-0.95, 0.95, (B, A)) if kind else rng.standard_normal((B, A))).astype(np.float32)
    _, lp0, _, v0 = O.get_action_and_value(L, p, x[:256], 1, act[:256])
    olp = (np.resize(lp0, B) + rng.standard_normal(B) * 0.1).astype(np.float32)
    ov = (np.resize(v0, B) + rng.standard_normal(B) * 0.1).astype(np.float32)
    adv = rng.standard_normal(B).astype(np.float32)
    ret = rng.standard_normal(B).astype(np.float32)
    perm = rng.permutation(B).astype(np.int32)
    grads, stats = [], []
    for opt in ("upd_kernel=fwdbwd", "upd_kernel=auto"):
        ag = make_agent(kind, O_, A, H, E, T=T, MB=1, EP=1, clip=0.1, options=opt)
        ag.load_params(p)
        fill_storage(ag, T, E, x, act, olp, adv, ret, ov)
        st = ag.update(2.5e-4, perms=DeviceArray.from_numpy(perm), want_stats=True)
        grads.append(ag.last_grad())
        stats.append([st[k] for k in ("pg_loss", "v_loss", "entropy", "approx_kl", "clipfrac", "grad_norm")])
        ag.close()
    assert rel(grads[1], grads[0]) < 2e-5
    for t in range(L.ntensors):
        o, n = L.t_off[t], L.t_len[t]
        if L.t_grad[t]:
            assert rel(grads[1][o:o + n], grads[0][o:o + n]) < 2e-4, t
    np.testing.assert_allclose(stats[1], stats[0], rtol=2e-5, atol=1e-7)


@pytest.mark.parametrize("O_,A,n", [(376, 17, 1000), (17, 6, 777), (11, 3, 5)])
def test_act_kernels_agree(O_, A, n):
    """The K-split two-trunk k_act4 and the feature-split k_act2 (64-wide tanh agent) give the same
    forward (summation order only) and, through the shared Philox contract, the same samples."""
    rng = np.random.default_rng(9)
    L = O.layout_init(0, O_, A, 64)
    p = random_params(L, rng)
    p[L.logstd:L.logstd + A] = -0.5
    x = rng.standard_normal((n, O_)).astype(np.float32)
    given = rng.standard_normal((n, A)).astype(np.float32)
    outs = []
    for opt in ("act_kernel=2", "act_kernel=4"):
        ag = make_agent(0, O_, A, 64, n, options=opt)
        ag.load_params(p)
        xd = DeviceArray.from_numpy(x)
        res = []
        for mode, ain in ((ppo_amd.PPO_SAMPLE, None), (ppo_amd.PPO_MEAN, None),
                          (ppo_amd.PPO_GIVEN, DeviceArray.from_numpy(given))):
            act, lp, ent, v = ag.get_action_and_value(xd, mode, ain, env_base=3, step_id=11)
            res.append([t.numpy() for t in (act, lp, ent, v)])
        outs.append(res)
        ag.close()
    for r2, r4 in zip(*outs):
        for t2, t4 in zip(r2, r4):
            np.testing.assert_allclose(t4, t2, rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("kind,O_,A,H,E", [(1, 17, 6, 256, 1599), (0, 17, 6, 256, 1599), (1, 9, 3, 256, 1599),
                                           (1, 17, 6, 256, 4100), (0, 376, 17, 64, 1599), (1, 105, 8, 256, 1599)])
def test_fused_dw_matches_two_phase_dw(kind, O_, A, H, E):
    """k_dwf (dW2 and dW1 in one pass over the rows), k_dwf_dma (the same, rows staged by LDS DMA in
    three buffers: create option dw_dma=1) and the two-phase k_dw run the same MFMA chains over the
    same rows in the same order: the gradients are bitwise equal (ragged last chunk and stage:
    M = 12 800 - 8 rows, output halves; M = 32 800, whole rows). The 64-wide agent at Humanoid's
    O = 376 compares k_dw2 (dw_dma=0) with k_dw2_dma (the default) the same way, and Ant's O = 105
    (OP = 112, the two-phase k_dw) k_dw with k_dw_dma."""
    rng = np.random.default_rng(7)
    L = O.layout_init(kind, O_, A, H)
    p = random_params(L, rng)
    if kind == 0:
        p[L.logstd:L.logstd + A] = -0.5
    T = 8
    B = T * E
    x = rng.standard_normal((B, O_)).astype(np.float32)
    act = (rng.uniform(-0.95, 0.95, (B, A)) if kind else rng.standard_normal((B, A))).astype(np.float32)
    olp = rng.standard_normal(B).astype(np.float32)
    ov = rng.standard_normal(B).astype(np.float32)
    adv = rng.standard_normal(B).astype(np.float32)
    ret = rng.standard_normal(B).astype(np.float32)
    perm = rng.permutation(B).astype(np.int32)
    grads = []
    # (fp32 MFMAs throughout: the default fused dW runs split-bf16 products, dw_mfma)
    for opt in ("dw_fused=0,dw_mfma=f32", "dw_dma=0", "dw_dma=1,dw_mfma=f32"):
        ag = make_agent(kind, O_, A, H, E, T=T, MB=1, EP=1, clip=0.1, options=opt)
        ag.load_params(p)
        fill_storage(ag, T, E, x, act, olp, adv, ret, ov)
        ag.update(2.5e-4, perms=DeviceArray.from_numpy(perm), want_stats=True)
        grads.append(ag.last_grad())
        ag.close()
    assert np.isfinite(grads[0]).all()
    np.testing.assert_array_equal(grads[1], grads[0])
    np.testing.assert_array_equal(grads[2], grads[0])


def test_cfg1_shape_iteration_vs_oracle():
    """BASELINE cfg1's shape (ppo_continuous_action defaults, ppo:57-66: num_envs=1, num_steps=2048,
    32 minibatches of 64 rows, 10 epochs): one full iteration -- 2048 batch-1 rollout acts on the
    device env, GAE over T=2048 for one env, 320 optimizer steps -- against the oracle doing the
    same with the same Philox counters and Feistel permutations. The rollout is checked against
    the oracle's rollout; the update against the oracle's update of the GPU's own rollout buffers
    (identical inputs: 2048 env steps would otherwise feed ulp-level action differences into 320
    chained Adam steps). The Adam chain still lets fp32 rounding differences grow, hence atol 1e-4
    on the parameters (lr 3e-4 per step)."""
    E, T, MB, EP = 1, 2048, 32, 10
    O_, A, H = 17, 6, 64
    rng = np.random.default_rng(23)
    L = O.layout_init(0, O_, A, H)
    p = random_params(L, rng)
    p[L.logstd:L.logstd + A] = -0.5
    cfg = ppo_amd.PPOConfig(num_envs=E, num_steps=T, num_minibatches=MB, update_epochs=EP, env_id="HalfCheetah-v5",
                            total_timesteps=E * T * 2, ent_coef=0.0)
    tr = ppo_amd.Trainer(cfg, params=p)
    tr.iterate()
    gpu_p = tr.agent.params()
    gpu_obs = tr.agent.buffer(ppo_amd.BUF_OBS, (T, E, O_)).numpy()
    gpu_adv = tr.agent.buffer(ppo_amd.BUF_ADVANTAGES, (T, E)).numpy()
    gb = {k: tr.agent.buffer(b, (T, E)).numpy() for k, b in (("logp", ppo_amd.BUF_LOGPROBS),
                                                              ("ret", ppo_amd.BUF_RETURNS),
                                                              ("val", ppo_amd.BUF_VALUES))}
    gpu_act = tr.agent.buffer(ppo_amd.BUF_ACTIONS, (T, E, A)).numpy()
    oenv = O.SynthEnv(E, O_, A, wrappers=True, gamma=cfg.gamma)  # ppo:41-49 wrapper chain, as the Trainer
    nobs = oenv.reset(cfg.seed)
    ndone = np.zeros(E, np.float32)
    bo = np.zeros((T, E, O_), np.float32); ba = np.zeros((T, E, A), np.float32)
    bl = np.zeros((T, E), np.float32); br = np.zeros((T, E), np.float32)
    bd = np.zeros((T, E), np.float32); bv = np.zeros((T, E), np.float32)
    for t in range(T):
        bo[t] = nobs; bd[t] = ndone
        a, lp, _, v = O.get_action_and_value(L, p, nobs, 0, seed=cfg.seed, rank=0, env_base=0, step_id=t)
        ba[t] = a; bl[t] = lp; bv[t] = v
        nobs, r, te, trn, _, _ = oenv.step(a)
        br[t] = r
        ndone = np.maximum(te, trn)
    assert bd.sum() >= 2  # the 1000-step truncation and its autoreset happen inside the rollout
    np.testing.assert_allclose(tr.agent.buffer(ppo_amd.BUF_REWARDS, (T, E)).numpy(), br, rtol=1e-3, atol=1e-4)
    _, _, _, nv = O.get_action_and_value(L, p, nobs, 2)
    adv, ret = O.gae(br, bv, bd, nv, ndone, 0.99, 0.95)
    # the obs are normalised by the wrapper chain: 1 / sqrt(var) scales the ulp-level action / dynamics
    # differences of 2 048 steps up by ~10 where the running variance is small
    np.testing.assert_allclose(gpu_obs, bo, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(gpu_adv, adv, rtol=1e-3, atol=1e-3)
    lcfg = O.LossCfg(0.2, 0.0, 0.5, 1, 1)
    lr = float(np.float32(cfg.learning_rate))
    np.testing.assert_allclose(gpu_act, ba, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(gb["logp"], bl, rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(gb["ret"], ret, rtol=1e-3, atol=1e-3)
    op, _, _, _, _ = O.update(L, p, np.zeros(L.P), np.zeros(L.P), 0, gpu_obs.reshape(-1, O_), gpu_act.reshape(-1, A),
                              gb["logp"].reshape(-1), gpu_adv.reshape(-1), gb["ret"].reshape(-1),
                              gb["val"].reshape(-1), EP, MB, lr, 0.5, 1e-5, lcfg, seed=cfg.seed, rank=0,
                              epoch_counter0=0)
    np.testing.assert_allclose(gpu_p, op, rtol=0, atol=1e-4)
    assert np.abs(gpu_p - p).max() > 1e-3  # 320 steps actually moved the parameters
    tr.close()


@pytest.mark.parametrize("net_kind,hidden,env_id,O_", [(1, 256, "HalfCheetah-v5", 17), (1, 256, "Ant-v5", 105),
                                                       (0, 64, "Humanoid-v4", 376)])
def test_weight_copies_track_adam(net_kind, hidden, env_id, O_):
    """k_act3 / k_act4 / k_upd / k_upd2 read W1, W2 and W2^T from transposed and MFMA-order
    (swizzled) copies that k_adam rewrites next to every parameter update. After a full iteration
    (16 or 64 Adam steps), act and value outputs computed from the incrementally maintained copies
    must equal, bitwise, those after the copies are rebuilt from the parameters (ppo_load_params
    -> k_transpose / k_swizzle), and so must one more update from the same parameters and Adam state
    (which also reads the split-bf16 pieces of the AC agent's k_upd)."""
    E, T = 256, 16
    C = ppo_amd.ACPPOConfig if net_kind == 1 else ppo_amd.PPOConfig
    cfg = C(num_envs=E, num_steps=T, num_minibatches=4, update_epochs=4, env_id=env_id, net_kind=net_kind,
            hidden=hidden, total_timesteps=E * T * 4)
    tr = ppo_amd.Trainer(cfg)
    p0 = tr.agent.params()
    tr.iterate()
    p1 = tr.agent.params()
    assert not np.array_equal(p0, p1)
    m1, v1, s1 = tr.agent.adam_state()
    x = DeviceArray.from_numpy(np.random.default_rng(9).standard_normal((E, O_)).astype(np.float32))
    outs, upd = [], []
    for rebuild in (False, True):
        if rebuild:
            tr.agent.load_params(p1)
            tr.agent.load_adam(m1, v1, s1)
        m, lp, ent, v = tr.agent.get_action_and_value(x, sample_type=ppo_amd.PPO_MEAN)
        outs.append([m.numpy(), lp.numpy(), ent.numpy(), v.numpy(), tr.agent.get_value(x).numpy()])
        # one more update over the stored rollout from the same state: k_upd / k_upd2 read the copies
        # too (the AC agent's default k_upd also the split-bf16 pieces of W2 | W2^T, bx_index)
        tr.agent.set_iteration(1)
        upd.append((tr.agent.update(1e-4), tr.agent.params()))
    for a, b in zip(*outs):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)
    (sa, pa), (sb, pb) = upd
    assert not np.array_equal(pa, p1)
    np.testing.assert_array_equal(pa, pb)
    assert sa == sb
    tr.close()


def test_values_bx_vs_oracle_at_metric_size():
    """The rollout's critic pass at the metric shape (T x E = 128 x 4 096, AC HalfCheetah 2 x 256):
    k_vbx (values_mfma=auto: layer 2 as six split-bf16 piece products, fp32 accumulation) over the
    stored observations of a persistent rollout, against the fp64-accumulating C oracle's critic on
    4 096 sampled rows (ac:655 values[step], the agent module ac:150-249), at the act tests' value bar
    (rtol 2e-5, atol 2e-5). The fp32-MFMA critic of the API act kernel (k_act3) runs the same rows and
    both errors are printed; the split form must stay within 2x of the fp32 form's error + 1e-6."""
    E, T = 4096, 128
    cfg = ppo_amd.ACPPOConfig(env_id="HalfCheetah-v5", num_envs=E, num_steps=T, total_timesteps=E * T * 2)
    tr = ppo_amd.Trainer(cfg)
    try:
        assert tr.agent.kernel_info().startswith("update=k_upd/bx6")
        tr.rollout()
        tr.agent.sync()
        O_ = 17
        obs = tr.agent.buffer(ppo_amd.BUF_OBS, (T, E, O_)).numpy().reshape(-1, O_)
        vals = tr.agent.buffer(ppo_amd.BUF_VALUES, (T, E)).numpy().reshape(-1)
        rng = np.random.default_rng(31)
        idx = np.sort(rng.choice(T * E, 4096, replace=False))
        x = np.ascontiguousarray(obs[idx])
        p = tr.agent.params()
        L = O.layout_init(1, O_, 6, 256)
        _, _, _, ov = O.get_action_and_value(L, p, x, 2)
        f32v = tr.agent.get_value(DeviceArray.from_numpy(x)).numpy()
    finally:
        tr.close()
    eb, ef = np.abs(vals[idx] - ov), np.abs(f32v - ov)
    print(f"\ncritic vs oracle, max |d|: k_vbx (bx6) {eb.max():.2e}, k_act3 (fp32 MFMA) {ef.max():.2e}; "
          f"rms {np.sqrt((eb ** 2).mean()):.2e} / {np.sqrt((ef ** 2).mean()):.2e}")
    np.testing.assert_allclose(vals[idx], ov, rtol=2e-5, atol=2e-5)
    assert np.sqrt((eb ** 2).mean()) <= 2 * np.sqrt((ef ** 2).mean()) + 1e-6
