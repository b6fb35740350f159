"""ReacherPlanar-v0 on the device (env kind PSYN_REACHER, include/ppo_synth_env.h) through the C-ABI:
the first real task with a two-dimensional action (O = 10, A = 2), a two-link planar arm with
Reacher-v5's task definition over the textbook two-link equations (not MuJoCo's Reacher). Each episode
has a goal of its own, env state that no step touches and every autoreset redraws.

  1. the per-step device env (k_env_reset<PSYN_REACHER> / k_env_step<PSYN_REACHER>) is the host env gymcpp/reacher.h bit for
     bit, without and with the PPO wrapper chain;
  2. the persistent rollouts (k_rollout, k_rollout4 at 4 and at 16 envs per workgroup) are the
     per-step path bit for bit, over two launches (T = 120, then T = 30 from the state the first left);
  3. the persistent evaluation (k_eval) is the per-step evaluation bit for bit, and both are what a
     step-by-step replay through the public calls gives;
  4. rollout_kernel=valu is refused for this env kind; the default options take the persistent path;
  5. one iteration of both agents against the CPU oracle;
  6. both CLIs run the task with host envs and with the device env;
  7. the trainer learns the task, with the PPO agent and with the AC agent (bars from the CPU
     reference runs, tests/golden/reacher).

Shapes: E = 37 (neither the 4-env nor the 16-env workgroup divides it), T = 120 (two autoresets, at
steps 50 and 101, inside one launch), T = 30 after it (an episode spans two launches). k_rollout4 takes
16 envs per workgroup only beyond 4 envs per CU, so its 16-env case runs at E = 4 CUs + 5 (odd).
"""
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import reacher_common as rc

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

ROOT = rc.ROOT
PKG = os.path.join(ROOT, "ppo.cpp_amd")
MODELS = os.path.join(PKG, "models")
ENV, OD, AD = rc.ENV_ID, rc.OD, rc.AD


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return rc.build_driver(str(tmp_path_factory.mktemp("reach") / "reacher_driver"))


# ------------------------------------------------------------------------------------------------
# 1. device per-step env == host env
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrapped", [False, True])
def test_device_env_bitwise_equals_host_env(driver, tmp_path, wrapped):
    """E = 37 (a ragged last block), T = 120 + 30, seed 6, actions uniform in [-3, 3]^2 (beyond the
    action space). Without wrappers everything is bitwise; with the PPO chain at gamma = 0.99 the
    normalised observations are within 1 ulp and rewards, dones and episode statistics are bitwise
    (test_gpu_wrappers.py's bars)."""
    E, T, seed = rc.GPU_E, rc.GPU_T + rc.GPU_T2, rc.GPU_SEED
    act = rc.gpu_actions()
    _, h0, h = rc.host_vec(driver, tmp_path, E, T, seed, "h", act, gamma=0.99 if wrapped else None)
    hdone = np.maximum(h["term"], h["trunc"])
    assert not h["term"].any() and sorted(set(np.nonzero(hdone)[0].tolist())) == [49, 100]
    env = ppo_amd.SynthEnv(E, env_id=ENV)
    assert env.info() == (ppo_amd.PSYN_REACHER, OD, AD, 50) and (env.O, env.A) == (OD, AD)
    w = None
    if wrapped:
        w = ppo_amd.EnvWrappers(E, OD, 0.99)
        env.attach_wrappers(w)
    obs, done, rew = DeviceArray((E, OD)), DeviceArray(E), DeviceArray(E)
    env.reset(seed, obs, done)
    env.episode_stats()

    def same_obs(a, b, msg):
        if wrapped:
            np.testing.assert_array_max_ulp(a, b, maxulp=1)
        else:
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=msg)

    same_obs(obs.numpy(), h0, "reset")
    assert (done.numpy() == 0).all()
    fin_ret, fin_len, fin_cnt = np.zeros(E, np.float32), np.zeros(E, np.float32), 0.0
    goals = []
    for t in range(T):
        env.step(DeviceArray.from_numpy(act[t]), obs, rew, done, lo=-1.0, hi=1.0)
        o = obs.numpy()
        same_obs(o, h["obs"][t], f"obs, step {t}")
        goals.append(o[:, 4:6].copy())
        np.testing.assert_array_equal(rew.numpy().view(np.uint32), h["rew"][t].view(np.uint32), err_msg=f"reward, step {t}")
        np.testing.assert_array_equal(done.numpy(), hdone[t], err_msg=f"done, step {t}")
        fin = h["len"][t] > 0
        fin_ret[fin] = (fin_ret[fin] + h["ret"][t][fin]).astype(np.float32)
        fin_len[fin] += h["len"][t][fin]
        fin_cnt += fin.sum()
    assert fin_cnt == 2 * E
    sr, sl, n = env.episode_stats()
    assert (np.float32(sr), sl, n) == (np.float32(fin_ret.astype(np.float64).sum()), fin_len.sum(), fin_cnt)
    if not wrapped:  # the goal survives every step and is redrawn at the resets (steps 50 and 101)
        goals = np.stack(goals)
        for a, b in ((0, 50), (50, 101), (101, T)):
            assert (goals[a:b] == goals[a]).all()
        assert (goals[49] != goals[50]).all() and (goals[100] != goals[101]).all()
    env.close()
    if w is not None:
        w.close()


# ------------------------------------------------------------------------------------------------
# 2. persistent rollout == per-step rollout
# ------------------------------------------------------------------------------------------------
BUFS = [("obs", "BUF_OBS", 1), ("actions", "BUF_ACTIONS", 2), ("logp", "BUF_LOGPROBS", 0),
        ("rewards", "BUF_REWARDS", 0), ("dones", "BUF_DONES", 0), ("values", "BUF_VALUES", 0)]


def snapshot(tr, agent=None):
    agent = agent or tr.agent
    E, T, O_, A = agent.hcfg.num_envs, agent.hcfg.num_steps, agent.hcfg.obs_dim, agent.hcfg.act_dim
    out = {}
    for name, b, kind in BUFS:
        shape = (T, E, O_) if kind == 1 else (T, E, A) if kind == 2 else (T, E)
        out[name] = agent.buffer(getattr(ppo_amd, b), shape).numpy()
    out["next_obs"] = tr.next_obs.numpy()
    out["next_done"] = tr.next_done.numpy()
    return out


def _cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _advance(tr, steps, seed=21):
    """`steps` per-step env steps (k_env_step<PSYN_REACHER>, through the wrapper chain where attached) with actions
    uniform in [-3, 3]^2, into the trainer's next_obs / next_done."""
    E = tr.hcfg.num_envs
    act = np.random.default_rng(seed).uniform(-3, 3, (steps, E, AD)).astype(np.float32)
    rew = DeviceArray(E)
    for t in range(steps):
        tr.env.step(DeviceArray.from_numpy(act[t]), tr.next_obs, rew, tr.next_done, lo=-1.0, hi=1.0)
    rew.numpy()  # a blocking copy: the steps have run before the rollout starts on the agent's stream
    tr.agent.sync()


def _assert_equal(snaps, what):
    for k in snaps[0]:
        np.testing.assert_array_equal(snaps[0][k].view(np.uint32), snaps[1][k].view(np.uint32), err_msg=f"{what}: {k}")


def _assert_rollout_pair_equal(cfg, opts, T2=rc.GPU_T2, update=True):
    """Two trainers (persistent, per-step) of one config: the rollout of cfg.num_steps steps, GAE and
    one update, then a second rollout of T2 steps from the state the first left (a second context of
    num_steps = T2 with the trainer's parameters, on the trainer's env, next_obs and next_done), then
    three more env steps with given actions. Everything is compared bitwise. Returns the snapshots of
    the persistent path."""
    trs = [ppo_amd.Trainer(cfg, options=o) for o in opts]
    E = cfg.num_envs
    try:
        assert trs[0].env.info()[0] == ppo_amd.PSYN_REACHER
        snaps, stats = [], []
        for tr in trs:
            tr.rollout()
            tr.agent.sync()
            snaps.append(snapshot(tr))
            stats.append(tr.env.episode_stats())
            if update:
                tr.agent.compute_gae(tr.next_obs, tr.next_done)
                tr.agent.update(tr.lr_now(), want_stats=False)
                tr.agent.sync()
        _assert_equal(snaps, "first rollout")
        assert stats[0] == stats[1] and stats[0][2] > 0
        np.testing.assert_array_equal(trs[0].agent.params(), trs[1].agent.params())
        first = snaps[0]
        # the second launch: the episodes that were under way go on
        snaps2, stats2 = [], []
        hc2 = ppo_amd.hip_config(dataclasses.replace(cfg, num_steps=T2, total_timesteps=E * T2))
        for tr, o in zip(trs, opts):
            ag = ppo_amd.Agent(hc2, options=o)
            try:
                ag.load_params(tr.agent.params())
                ppo_amd.check(ppo_amd.lib().ppo_rollout_synth(ag.h, tr.env.h, tr.next_obs.ptr, tr.next_done.ptr,
                                                               tr.act_scratch.ptr, tr.rew_scratch.ptr))
                ag.sync()
                snaps2.append(snapshot(tr, ag))
                stats2.append(tr.env.episode_stats())
            finally:
                ag.close()
        _assert_equal(snaps2, "second rollout")
        assert stats2[0] == stats2[1]
        # the env state both left behind (angles, speeds, goal, step count, reset count, autoreset
        # flag): three more env steps with the same actions give the same bits
        outs = []
        for tr in trs:
            rew = DeviceArray(E)
            seq = []
            for k in range(3):
                a = np.stack([np.linspace(-1.5, 1.5, E), np.linspace(0.7, -1.2, E)], 1).astype(np.float32) * (k + 1)
                tr.env.step(DeviceArray.from_numpy(a), tr.next_obs, rew, tr.next_done, lo=-1.0, hi=1.0)
                seq += [tr.next_obs.numpy(), rew.numpy(), tr.next_done.numpy()]
            outs.append(seq)
        for x, y in zip(*outs):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
        if trs[0].wrappers is not None:
            for k, v in trs[0].wrappers.state().items():
                np.testing.assert_array_equal(v, trs[1].wrappers.state()[k], err_msg=k)
        return first, snaps2[0], outs[0]
    finally:
        for tr in trs:
            tr.close()


@pytest.mark.parametrize("agent,shape", [("ac", "E37"), ("ppo", "E37"), ("ppo", "4CU+5")])
def test_persistent_rollout_bitwise_equals_per_step(agent, shape):
    """AC agent: k_rollout<1, 1, PSYN_REACHER> + k_values vs k_act3 + k_env_step<PSYN_REACHER>. PPO agent with the
    wrapper chain: k_rollout4 at 4 envs per workgroup (E = 37) and at 16 (E = 4 CUs + 5: more 4-env
    workgroups than CUs) vs k_act4 + k_env_step<PSYN_REACHER>. T = 120 holds the autoresets of steps 50 and 101;
    the second launch (T = 30) continues the third episode, which ends on the second of the three env
    steps after it. Compared: all storage buffers, next_obs / next_done, the env state (the steps
    after; the goal is part of every observation), the wrapper state, the episode sums and the
    parameters after an update. The two action columns of the stored actions differ in more than 99 %
    of the rows: a kernel that fed action 0 twice would not pass as the per-step path's equal."""
    E = 37 if shape == "E37" else 4 * _cu_count() + 5
    assert E % 4 and E % 16
    T = rc.GPU_T
    C = ppo_amd.ACPPOConfig if agent == "ac" else ppo_amd.PPOConfig
    cfg = C(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=2, update_epochs=1, total_timesteps=E * T * 2)
    first, second, after = _assert_rollout_pair_equal(cfg, ["act_kernel=4", "act_kernel=4,rollout=per_step"])
    for s in (first, second):
        assert np.isfinite(s["values"]).all() and np.isfinite(s["logp"]).all()
        a = s["actions"].reshape(-1, AD)
        assert (a[:, 0] != a[:, 1]).mean() > 0.99
    # dones [t] is the done flag going into step t: the truncations of steps 49 and 100
    assert sorted(set(np.nonzero(first["dones"].any(1))[0].tolist())) == [50, 101]
    assert (first["dones"][50] == 1).all() and (first["rewards"][[50, 101]] == 0).all()
    assert not second["dones"].any() and not second["next_done"].any()
    assert (after[2] == 0).all() and (after[5] == 1).all() and (after[8] == 0).all()  # step 50 of the third episode
    if agent == "ac":
        assert np.abs(first["actions"]).max() <= 1.0
        g = first["obs"][:, :, 4:6]  # unwrapped: the goal is constant within an episode, new after a reset
        for a0, b0 in ((0, 50), (51, 101), (102, T)):
            assert (g[a0:b0] == g[a0]).all()
        assert (g[49] != g[51]).all() and (g[100] != g[102]).all()
        np.testing.assert_array_equal(second["obs"][:, :, 4:6], np.broadcast_to(g[T - 1], second["obs"][:, :, 4:6].shape))


# ------------------------------------------------------------------------------------------------
# 3. evaluation
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ac_agent():
    hc = ppo_amd.HipConfig(ppo_amd.PPO_NET_LN_BETA, OD, AD, 256, 64, 4, 1, 1, 0.99, 0.95, 0.2, 0.01, 0.5, 0.5, 1e-5, 1, 1, 1, 0, 1)
    ag = ppo_amd.Agent(hc)
    ag.load_params(ppo_amd.init_params(ag.layout, seed=3, env_id=ENV))
    yield ag
    ag.close()


def _replay_events(agent, env, E, nE, runs, mode, eval_seed, step0):
    """The evaluation through the public per-step calls: reset(eval_seed), then act on envs [0, nE),
    psyn_step, and one event (step, env, length, return) per done; stops after the step at which the
    event count reaches `runs`, keeping all events of that step, in (step, env) order."""
    obs, done, rew = DeviceArray((E, OD)), DeviceArray(E), DeviceArray(E)
    env.reset(eval_seed, obs, done)
    x = DeviceArray.wrap(obs.ptr, (nE, OD))
    events, length, fresh, k = [], np.zeros(nE, np.int64), np.zeros(nE, bool), 0
    ret = np.zeros(nE, np.float32)
    while len(events) < runs:
        act, _, _, _ = agent.get_action_and_value(x, mode, step_id=step0 + k)
        env.step(act, obs, rew, done, lo=-1.0, hi=1.0, e0=0, e1=nE)
        d = done.numpy()[:nE] != 0
        length = np.where(fresh, 0, length + 1)  # the step after a done is the reset step
        ret = np.where(fresh, np.float32(0), (ret + rew.numpy()[:nE]).astype(np.float32)).astype(np.float32)
        events += [(k, int(e), int(length[e]), float(ret[e])) for e in np.nonzero(d)[0]]
        fresh = d
        k += 1
        assert k < 200
    return events, k


@pytest.mark.parametrize("name,mode", [("mean", ppo_amd.PPO_MEAN), ("roach", ppo_amd.PPO_ROACH), ("sample", ppo_amd.PPO_SAMPLE)])
@pytest.mark.parametrize("nE", [1, 19])
def test_eval_kernel_bitwise_equals_per_step(ac_agent, name, mode, nE):
    """num_eval_envs = 1 and = E; chunk_steps = 50 (an episode per chunk, the reset step opens the
    next) and 23 (does not divide 50); the chunk size changes no returned bit. Two episodes per env:
    the second has a goal of its own."""
    E = 19
    runs = 2 if nE == 1 else E + 1
    env = ppo_amd.SynthEnv(E, env_id=ENV)
    step0 = (1 << 40) if name == "sample" else 0
    fast = ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0, chunk_steps=50)
    assert ac_agent.eval_info() == "eval=k_eval"
    odd = ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0, chunk_steps=23)
    assert ac_agent.eval_info() == "eval=k_eval"
    slow = ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0, chunk_steps=50, per_step=True)
    assert ac_agent.eval_info() == "eval=per_step"
    dflt = ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0)
    events, steps = _replay_events(ac_agent, env, E, nE, runs, mode, 2, step0)
    env.close()
    for other in (odd, slow, dflt):
        np.testing.assert_array_equal(fast[0].view(np.uint32), other[0].view(np.uint32))
        np.testing.assert_array_equal(fast[1], other[1])
        assert fast[2] == other[2]
    print(f"{name} nE={nE}: {len(events)} events, env steps {steps}, returns {fast[0][:4]}")
    assert events == sorted(events) and fast[2] == steps == 101
    assert len(events) == 2 * nE and {k for k, _, _, _ in events} == {49, 100}
    np.testing.assert_array_equal(fast[1], [ln for _, _, ln, _ in events])
    np.testing.assert_array_equal(fast[0].view(np.uint32), np.asarray([r for _, _, _, r in events], np.float32).view(np.uint32))
    assert (fast[1] == 50).all() and (fast[0] < 0).all()
    assert len(set(fast[0].tolist())) == len(fast[0])  # every episode has its own goal and so its own return


# ------------------------------------------------------------------------------------------------
# 4. kernel selection
# ------------------------------------------------------------------------------------------------
def test_valu_rollout_is_refused_and_default_is_persistent():
    E, T = 64, 60
    cfg = ppo_amd.ACPPOConfig(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=2, update_epochs=1,
                              total_timesteps=E * T * 2)
    tr = ppo_amd.Trainer(cfg, options="rollout_kernel=valu")
    try:
        with pytest.raises(ppo_amd.PPOError, match=r"rollout_kernel=valu.*PSYN_REACHER"):
            tr.rollout()
    finally:
        tr.close()
    tr = ppo_amd.Trainer(cfg)
    try:
        # the persistent rollout leaves the values to a pass of their own; "values=k_act" is the
        # per-step path's answer
        info = tr.agent.kernel_info()
        assert "values=k_v" in info and "values=k_act" not in info, info
    finally:
        tr.close()
    # E = 64 <= 512: the synthetic cheetah would take k_rollout_v here; this kind takes k_rollout
    first, _, _ = _assert_rollout_pair_equal(cfg, [None, "rollout=per_step"], T2=5)
    assert first["dones"].sum() == E


# ------------------------------------------------------------------------------------------------
# 5. one iteration against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_one_iteration_vs_oracle(kind):
    """One iteration (E = 16, T = 16, one minibatch, one epoch) against the oracle with the bars of
    test_gpu_cartpole.py::test_one_iteration_vs_oracle: teacher-forced act per stored step (A = 2: the
    summed log-probability), GAE bit-exact, loss statistics (the summed entropy among them) and
    parameters after one Adam step. The envs first take 40 per-step env steps, so the truncation of
    step 50 and the reset after it fall inside the 16 stored steps."""
    E, T, H = 16, 16, (64 if kind == 0 else 256)
    C = ppo_amd.PPOConfig if kind == 0 else ppo_amd.ACPPOConfig
    cfg = C(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=1, update_epochs=1, total_timesteps=E * T * 4, seed=3)
    L = O.layout_init(kind, OD, AD, H)
    tr = ppo_amd.Trainer(cfg)
    try:
        p0 = tr.agent.params().copy()
        assert p0.size == L.P
        _advance(tr, 40)
        tr.rollout()
        tr.agent.sync()
        g = snapshot(tr)
        nv = tr.agent.get_value(tr.next_obs)
        tr.agent.gae_from_values(nv, tr.next_done)
        nv = nv.numpy().reshape(E)
        gadv = tr.agent.buffer(ppo_amd.BUF_ADVANTAGES, (T, E)).numpy()
        gret = tr.agent.buffer(ppo_amd.BUF_RETURNS, (T, E)).numpy()
        lr = tr.lr_now()
        st = tr.agent.update(lr, want_stats=True)
        gpu_p = tr.agent.params()
    finally:
        tr.close()
    assert g["dones"].sum() == E and (g["dones"][10] == 1).all()  # step 50 was stored step 9
    bad = 0
    for t in range(T):
        a, lp, _, v = O.get_action_and_value(L, p0, g["obs"][t], 0, seed=cfg.seed, rank=0, env_base=0, step_id=t)
        close = np.isclose(g["actions"][t], a, rtol=1e-4, atol=1e-4).all(axis=1)
        close &= np.isclose(g["logp"][t], lp, rtol=1e-4, atol=1e-3)
        close &= np.isclose(g["values"][t], v, rtol=2e-5, atol=2e-5)
        bad += int((~close).sum())
    assert bad <= max(1, 1e-4 * T * E), bad
    _, _, _, onv = O.get_action_and_value(L, p0, g["next_obs"], 2)
    np.testing.assert_allclose(nv, onv, rtol=2e-5, atol=2e-5)
    oadv, oret = O.gae(g["rewards"], g["values"], g["dones"], nv, g["next_done"], cfg.gamma, cfg.gae_lambda)
    np.testing.assert_array_equal(gadv, oadv)
    np.testing.assert_array_equal(gret, oret)
    lcfg = O.LossCfg(cfg.clip_coef, cfg.ent_coef, cfg.vf_coef, int(cfg.clip_vloss), int(cfg.norm_adv))
    op, _, _, _, ost = O.update(L, p0, np.zeros(L.P), np.zeros(L.P), 0, g["obs"].reshape(-1, OD), g["actions"].reshape(-1, AD),
                                g["logp"].reshape(-1), gadv.reshape(-1), gret.reshape(-1), g["values"].reshape(-1), 1, 1,
                                lr, cfg.max_grad_norm, cfg.adam_eps, lcfg, seed=cfg.seed, rank=0, epoch_counter0=0)
    got = [st["pg_loss"], st["v_loss"], st["entropy"], st["old_approx_kl"], st["approx_kl"], st["clipfrac"]]
    print("stats gpu", got, "oracle", ost[:6].tolist(), "params max |d|", np.abs(gpu_p.astype(np.float64) - op).max())
    np.testing.assert_allclose(got, ost[:6], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(gpu_p, op, rtol=0, atol=2e-6)


# ------------------------------------------------------------------------------------------------
# 6. CLIs
# ------------------------------------------------------------------------------------------------
def _run(args, timeout=240):
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("exe,kind,H", [("ac_ppo_continuous_action", ppo_amd.PPO_NET_LN_BETA, 256),
                                        ("ppo_continuous_action", ppo_amd.PPO_NET_TANH_NORMAL, 64)])
def test_cli_host_and_device_env(exe, kind, H):
    """--env_id ReacherPlanar-v0 with host envs (gymcpp::ReacherPlanar; the PPO trainer's behind the
    wrapper chain) and with the device env: 2 envs, 2 iterations of 64 steps. Both print the evaluation
    lines and save finite weights of the agent's size; the AC trainer (no wrappers: host and device
    envs agree bit for bit) ends with the same weights on both backends, and its mean-action
    evaluation on env 0 prints the same lines."""
    E, T = 2, 64
    common = ["--env_id", ENV, "--num_envs", str(E), "--num_steps", str(T), "--total_timesteps", str(E * T * 2),
              "--seed", "4", "--num_eval_runs", "2"]
    path = os.path.join(PKG, "bin", exe)
    outs, params = {}, {}
    L = ppo_amd.agent_layout(kind, OD, AD, H)
    for backend in ("host", "device"):
        outs[backend] = _run([path, "--env_backend", backend, "--exp_name_stem", f"t_reach_{exe[:2]}_{backend}"] + common)
        assert "Average evaluation return=" in outs[backend]
        p = ppo_amd.load_agent_pth(L, os.path.join(MODELS, f"t_reach_{exe[:2]}_{backend}_4", "model_final.pth"))
        assert p.size == L.P and np.isfinite(p).all()
        params[backend] = p
    ev = {k: [ln for ln in v.splitlines() if ln.startswith("Evaluation result")] for k, v in outs.items()}
    # (ppo_continuous_action on the device env prints the average line alone, for every env id)
    assert len(ev["host"]) == 2
    if exe.startswith("ac"):
        assert len(ev["device"]) == 2
        np.testing.assert_array_equal(params["host"], params["device"])
        assert ev["host"] == ev["device"]


# ------------------------------------------------------------------------------------------------
# 7. it learns
# ------------------------------------------------------------------------------------------------
def _learns(ref_name):
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reacher", ref_name)))
    c = ref["config"]
    assert ref["condition_met"] and ref["env_id"] == ENV and len(ref["seeds"]) == 3
    bar = 0.5 * min(r["trained"] - r["untrained"] for r in ref["runs"])
    assert bar > 0
    C = ppo_amd.PPOConfig if c["agent"] == "ppo" else ppo_amd.ACPPOConfig
    E = c["num_envs"]
    res = []
    for seed in ref["seeds"]:
        cfg = C(env_id=ENV, seed=seed, **{k: c[k] for k in ("num_envs", "num_steps", "total_timesteps", "num_minibatches",
                                                          "update_epochs", "learning_rate", "gamma", "gae_lambda", "clip_coef",
                                                          "ent_coef", "vf_coef", "max_grad_norm", "adam_eps")})
        tr = ppo_amd.Trainer(cfg)
        try:
            def evaluate():
                # one 50-step chunk: every env finishes its episode on the chunk's last step
                r, ln, _ = tr.agent.evaluate(tr.env, ref["eval_episodes"], ppo_amd.PPO_MEAN, eval_seed=c["eval_seed"],
                                             num_eval_envs=E, chunk_steps=50)
                assert r.size >= ref["eval_episodes"] and (ln == 50).all()
                return float(r.astype(np.float64).mean())
            untrained = evaluate()
            tr.env.reset(cfg.seed, tr.next_obs, tr.next_done, ppo_amd.lib().ppo_stream(tr.agent.h))
            for _ in range(cfg.num_iterations):
                tr.iterate()
            trained = evaluate()
        finally:
            tr.close()
        print(f"{c['agent']} seed {seed}: untrained {untrained:.2f} -> trained {trained:.2f} "
              f"(improvement {trained - untrained:.2f}, bar {bar:.2f})")
        res.append((seed, untrained, trained))
    # the reference's own rule, on the GPU runs: every seed improves by twice the untrained spread
    spread = max(u for _, u, _ in res) - min(u for _, u, _ in res)
    for seed, untrained, trained in res:
        assert trained - untrained >= bar, (seed, untrained, trained, bar)
        assert trained - untrained >= 2 * spread, (seed, untrained, trained, spread)


def test_it_learns():
    """ppo_amd.Trainer (the PPO agent, wrapper chain on, k_rollout4 at A = 2) with the config and seeds
    of tests/golden/reacher/learning_ref.json (written by scripts/reacher_learning_ref.py: the same
    loop on the CPU from the oracle and the host env). Per seed, the improvement of the mean-action
    evaluation return (64 episodes, Agent.evaluate on all envs, one 50-step chunk) from before to
    after training must be at least half the smallest improvement of the reference, and at least twice
    the spread of the untrained returns: the GPU and CPU trajectories part at the first rounding
    difference, so what is compared is whether learning happens, not a curve.
    Measured (MI355X): seeds 1, 2, 3 improve by 2.59, 2.93, 1.97 (from -10.08 each); the reference by
    2.43, 3.02, 2.44; the bar is 1.21 and the untrained spread 0.004."""
    _learns("learning_ref.json")


def test_it_learns_ac():
    """The AC agent (LayerNorm-Beta, H = 256, no wrappers; k_rollout<1, 1, PSYN_REACHER>, evaluation by
    k_eval) with the config and seeds of tests/golden/reacher/learning_ref_ac.json, the same script's
    run with --agent ac --total_timesteps 491520 (60 iterations: with the PPO agent's 20 the reference
    improves by 1.09 to 1.46, less than twice the untrained spread 1.42), and the same bars.
    Measured (MI355X): seeds 1, 2, 3 improve by 3.65, 4.92, 3.98; the reference by 3.44, 4.87, 4.12;
    the bar is 1.72 and twice the untrained spread 2.84."""
    _learns("learning_ref_ac.json")
