"""QuadrotorHover-v0 on the device (env kind PSYN_QUADROTOR, include/ppo_synth_env.h) through the
C-ABI: the first real task on the two-tile kernels (O = 18, A = 4), a rigid-body quadrotor hovering at
the origin that terminates (|p|^2 > 9) and truncates (500 steps).

  1. the per-step device env (k_env_reset<PSYN_QUADROTOR> / k_env_step<PSYN_QUADROTOR>) is the host env gymcpp/quadrotor.h bit for
     bit over the desynchronised run of test_quadrotor_cpu.py, without and with the PPO wrapper chain
     (with it: against the oracle's chain, as test_gpu_cartpole.py does);
  2. the persistent rollouts (k_rollout<2, 1, PSYN_QUADROTOR>, k_rollout4<2, 1, ., PSYN_QUADROTOR> at 4
     and at 16 envs per workgroup) are the per-step path bit for bit, over two launches of T = 64;
  3. a truncation inside a persistent launch: 490 per-step steps under the scripted PD controller, then
     one launch of T = 32 that crosses step 500;
  4. the persistent evaluation (k_eval<2, 1, PSYN_QUADROTOR>) is the per-step evaluation bit for bit,
     and both are what a step-by-step replay through the public calls gives;
  5. rollout_kernel=valu is refused for this env kind; the default options take the persistent path;
  6. one iteration of both agents against the CPU oracle at O = 18, A = 4;
  7. both CLIs: host envs and the device env end with the same weights;
  8. the trainer learns the task, with the PPO agent and with the AC agent (bars from the CPU
     reference runs, tests/golden/quadrotor).

Shapes: E = 37 (neither the 4-env nor the 16-env workgroup divides it) and E = 5. k_rollout4 takes 16
envs per workgroup only beyond 4 envs per CU, so its 16-env case runs at E = 4 CUs + 5 (odd).
"""
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import quadrotor_common as qc

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

ROOT = qc.ROOT
PKG = os.path.join(ROOT, "ppo.cpp_amd")
MODELS = os.path.join(PKG, "models")
ENV, OD, AD = qc.ENV_ID, qc.OD, qc.AD


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return qc.build_driver(str(tmp_path_factory.mktemp("quad") / "quadrotor_driver"))


# ------------------------------------------------------------------------------------------------
# 1. device per-step env == host env
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrapped", [False, True])
def test_device_env_bitwise_equals_host_env(driver, tmp_path, wrapped):
    """The desynchronised run (E = 37: a ragged last block; T = 300; seed 5; actions uniform in
    [-1.5, 1.5]^4, beyond the action space). Without wrappers everything is bitwise: observations,
    rewards, dones, episode statistics, and so the state. With the PPO chain at gamma = 0.99 the
    normalised observations are within 1 ulp of the host chain's and rewards, dones and episode
    statistics are bitwise (test_gpu_wrappers.py's bars); the wrapper state after the run is the
    oracle's chain's, fed the host env's raw stream with its termination flags, bit for bit."""
    E, T, seed = qc.GPU_E, qc.GPU_T, qc.GPU_SEED
    act = qc.gpu_actions()
    _, h0, h = qc.host_vec(driver, tmp_path, E, T, seed, "h", act, gamma=0.99 if wrapped else None)
    hdone = np.maximum(h["term"], h["trunc"])
    assert h["term"].sum() >= 2 * E and hdone.any(1).sum() >= 50 and hdone.sum(0).min() >= 2
    env = ppo_amd.SynthEnv(E, env_id=ENV)
    assert env.info() == (ppo_amd.PSYN_QUADROTOR, OD, AD, 500) and (env.O, env.A) == (OD, AD)
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
    for t in range(T):
        env.step(DeviceArray.from_numpy(act[t]), obs, rew, done, lo=-1.0, hi=1.0)
        same_obs(obs.numpy(), h["obs"][t], f"obs, step {t}")
        np.testing.assert_array_equal(rew.numpy().view(np.uint32), h["rew"][t].view(np.uint32), err_msg=f"reward, step {t}")
        np.testing.assert_array_equal(done.numpy(), hdone[t], err_msg=f"done, step {t}")
        fin = h["len"][t] > 0
        fin_ret[fin] = (fin_ret[fin] + h["ret"][t][fin]).astype(np.float32)
        fin_len[fin] += h["len"][t][fin]
        fin_cnt += fin.sum()
    assert fin_cnt == hdone.sum() and fin_cnt >= 2 * E
    sr, sl, n = env.episode_stats()
    assert (np.float32(sr), sl, n) == (np.float32(fin_ret.astype(np.float64).sum()), fin_len.sum(), fin_cnt)
    if w is not None:
        _, r0, raw = qc.host_vec(driver, tmp_path, E, T, seed, "raw", act)
        ow = O.VecWrappers(E, OD, 0.99)
        ow.reset(r0)
        was_done = np.zeros(E, np.float32)
        for t in range(T):
            ow.step(raw["obs"][t], raw["rew"][t], raw["term"][t], was_done)
            was_done = np.maximum(raw["term"][t], raw["trunc"][t])
        st, ost = w.state(), ow.state()
        assert {"rew_acc", "rew_mean", "rew_var", "rew_count", "obs_count", "obs_mean", "obs_var"} <= set(st)
        for k in st:
            np.testing.assert_array_equal(np.asarray(st[k], np.float32).view(np.uint32),
                                          np.asarray(ost[k], np.float32).view(np.uint32), err_msg=k)
        assert np.asarray(st["obs_mean"]).size == E * OD  # 18 observation columns through the chain
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


def _feed(tr, act):
    """per-step env steps (k_env_step<PSYN_QUADROTOR>, through the wrapper chain where attached) with the given
    actions [steps, E, 4], into the trainer's next_obs / next_done"""
    E = tr.hcfg.num_envs
    rew = DeviceArray(E)
    for t in range(len(act)):
        tr.env.step(DeviceArray.from_numpy(np.ascontiguousarray(act[t], np.float32)), tr.next_obs, rew, tr.next_done,
                    lo=-1.0, hi=1.0)
    rew.numpy()  # a blocking copy: the steps have run before the rollout starts on the agent's stream
    tr.agent.sync()


def _assert_equal(snaps, what):
    for k in snaps[0]:
        np.testing.assert_array_equal(snaps[0][k].view(np.uint32), snaps[1][k].view(np.uint32), err_msg=f"{what}: {k}")


def _assert_rollout_pair_equal(cfg, opts, T2, update=True, prefix=None):
    """Two trainers (persistent, per-step) of one config: (after the per-step prefix of given actions,
    if any) the rollout of cfg.num_steps steps, GAE and one update, then a second rollout of T2 steps
    from the state the first left (a second context of num_steps = T2 with the trainer's parameters,
    on the trainer's env, next_obs and next_done), then three more env steps with given actions.
    Everything is compared bitwise. Returns the snapshots and episode statistics of the persistent path."""
    trs = [ppo_amd.Trainer(cfg, options=o) for o in opts]
    E = cfg.num_envs
    try:
        assert trs[0].env.info()[0] == ppo_amd.PSYN_QUADROTOR
        snaps, stats = [], []
        for tr in trs:
            if prefix is not None:
                _feed(tr, prefix)
                tr.env.episode_stats()
            tr.rollout()
            tr.agent.sync()
            snaps.append(snapshot(tr))
            stats.append(tr.env.episode_stats())
            if update:
                tr.agent.compute_gae(tr.next_obs, tr.next_done)
                tr.agent.update(tr.lr_now(), want_stats=False)
                tr.agent.sync()
        _assert_equal(snaps, "first rollout")
        assert stats[0] == stats[1]
        np.testing.assert_array_equal(trs[0].agent.params(), trs[1].agent.params())
        first = snaps[0]
        snaps2, stats2 = [], []
        if T2:
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
        # the env state both left behind (the 13 state floats, step count, reset count, autoreset
        # flag): three more env steps with the same actions give the same bits
        outs = []
        for tr in trs:
            rew = DeviceArray(E)
            seq = []
            for k in range(3):
                a = np.stack([np.linspace(-1.5, 1.5, E), np.linspace(0.7, -1.2, E), np.linspace(-0.3, 0.9, E),
                              np.linspace(1.1, -0.6, E)], 1).astype(np.float32) * (k + 1) / 2
                tr.env.step(DeviceArray.from_numpy(a), tr.next_obs, rew, tr.next_done, lo=-1.0, hi=1.0)
                seq += [tr.next_obs.numpy(), rew.numpy(), tr.next_done.numpy()]
            outs.append(seq)
        for x, y in zip(*outs):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
        if trs[0].wrappers is not None:
            for k, v in trs[0].wrappers.state().items():
                np.testing.assert_array_equal(v, trs[1].wrappers.state()[k], err_msg=k)
        return first, (snaps2[0] if T2 else None), stats[0], (stats2[0] if T2 else None)
    finally:
        for tr in trs:
            tr.close()


@pytest.mark.parametrize("agent,shape", [("ac", "E37"), ("ppo", "E37"), ("ppo", "4CU+5")])
def test_persistent_rollout_bitwise_equals_per_step(agent, shape):
    """AC agent: k_rollout<2, 1, PSYN_QUADROTOR> + k_values vs k_act3 + k_env_step<PSYN_QUADROTOR>. PPO agent with the
    wrapper chain: k_rollout4<2, 1, ., PSYN_QUADROTOR> at 4 envs per workgroup (E = 37) and at 16
    (E = 4 CUs + 5: more 4-env workgroups than CUs) vs k_act4 + k_env_step<PSYN_QUADROTOR>. Two consecutive launches of
    T = 64: under sampled actions the envs terminate on steps of their own inside them, and an episode
    spans the two launches. Compared: all storage buffers, next_obs / next_done, the env state (the
    steps after), the wrapper state, the episode sums and the parameters after an update. The four
    action columns of the stored actions differ pairwise in more than 99 % of the rows: a kernel that
    fed one action four times would not pass as the per-step path's equal."""
    E = 37 if shape == "E37" else 4 * _cu_count() + 5
    assert E % 4 and E % 16
    T = 64
    C = ppo_amd.ACPPOConfig if agent == "ac" else ppo_amd.PPOConfig
    cfg = C(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=2, update_epochs=1, total_timesteps=E * T * 2)
    first, second, st1, st2 = _assert_rollout_pair_equal(cfg, ["act_kernel=4", "act_kernel=4,rollout=per_step"], T2=T)
    for s in (first, second):
        assert np.isfinite(s["values"]).all() and np.isfinite(s["logp"]).all()
        a = s["actions"].reshape(-1, AD)
        for i in range(AD):
            for j in range(i + 1, AD):
                assert (a[:, i] != a[:, j]).mean() > 0.99
    alld = np.concatenate([first["dones"], second["dones"], second["next_done"][None]])
    ends = alld.any(1).sum()
    print(f"{agent} {shape}: finished episodes {st1[2]} + {st2[2]}, envs that finished one {int((alld.sum(0) > 0).sum())} of {E}, "
          f"steps on which an episode ended {int(ends)}")
    assert st1[2] + st2[2] > 0 and alld.sum() > 0      # some envs finish an episode inside the launches
    assert (alld.sum(0) > 0).sum() >= E // 2 and ends >= 10  # most do, on steps of their own
    rst = np.nonzero(alld[:-1])  # dones[t] = 1: step t is the reset step, reward 0
    assert (np.concatenate([first["rewards"], second["rewards"]])[rst] == 0).all()
    if agent == "ac":
        assert np.abs(first["actions"]).max() <= 1.0


# ------------------------------------------------------------------------------------------------
# 3. truncation inside a persistent launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agent", ["ac", "ppo"])
def test_truncation_inside_a_persistent_launch(agent):
    """E = 5. The scripted PD controller's actions over the host env (which the device env equals bit
    for bit, test 1) hold every env in the air for 490 per-step steps; then one launch of T = 32 under
    the agent's sampled actions crosses step 500: stored step 9 is the 500th step of every env, step 10
    its reset. Persistent == per-step bitwise, and the finished episodes are E episodes of length 500.
    (On the host env the hovering state of step 490 survives far more than 10 steps of any actions:
    from rest at the origin, full thrust on one side for 10 steps moves the vehicle by centimetres.)"""
    E, T, seed = 5, 32, 7
    C = ppo_amd.ACPPOConfig if agent == "ac" else ppo_amd.PPOConfig
    cfg = C(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=1, update_epochs=1, total_timesteps=E * T * 2, seed=seed)
    prefix, steps = qc.pd_prefix_actions(E, seed, 490)
    assert not np.stack([r[3] for r in steps]).any()  # nobody ends in the prefix
    first, _, st, _ = _assert_rollout_pair_equal(cfg, [None, "rollout=per_step"], T2=0, prefix=prefix)
    assert (first["dones"][10] == 1).all() and first["dones"].sum() == E and not first["next_done"].any()
    assert (first["rewards"][10] == 0).all() and (first["rewards"][:10] > 0).all()
    sr, sl, n = st
    assert n == E and sl == 500.0 * E and sr > 1000.0 * E


# ------------------------------------------------------------------------------------------------
# 4. evaluation
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
        assert k < 3000
    return events, k


@pytest.mark.parametrize("name,mode", [("mean", ppo_amd.PPO_MEAN), ("sample", ppo_amd.PPO_SAMPLE)])
@pytest.mark.parametrize("nE", [1, 5])
def test_eval_kernel_bitwise_equals_per_step(ac_agent, name, mode, nE):
    """num_eval_envs = 1 and = E = 5; chunk_steps = 48: several chunks (the chunk size changes no
    returned bit). The episodes terminate on steps of their own."""
    E, runs = 5, 6
    env = ppo_amd.SynthEnv(E, env_id=ENV)
    step0 = (1 << 40) if name == "sample" else 0
    fast = ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0, chunk_steps=48)
    assert ac_agent.eval_info() == "eval=k_eval"
    slow = ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0, chunk_steps=48, per_step=True)
    assert ac_agent.eval_info() == "eval=per_step"
    dflt = ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0)
    events, steps = _replay_events(ac_agent, env, E, nE, runs, mode, 2, step0)
    env.close()
    for other in (slow, dflt):
        np.testing.assert_array_equal(fast[0].view(np.uint32), other[0].view(np.uint32))
        np.testing.assert_array_equal(fast[1], other[1])
        assert fast[2] == other[2]
    print(f"{name} nE={nE}: events (step, env, length, return) {events}, env steps {steps}")
    assert events == sorted(events) and fast[2] == steps
    np.testing.assert_array_equal(fast[1], [ln for _, _, ln, _ in events])
    np.testing.assert_array_equal(fast[0].view(np.uint32), np.asarray([r for _, _, _, r in events], np.float32).view(np.uint32))
    assert len(set(fast[1].tolist())) > 1 and (fast[1] >= 10).all() and (fast[1] <= 500).all()
    assert (fast[0] > 0).all() and (fast[0] <= 3.0 * fast[1]).all()  # the reward lies in (0, 3]
    last = events[-1][0]
    on_last = sum(1 for k, _, _, _ in events if k == last)
    assert len(events) - on_last < runs <= len(events)


# ------------------------------------------------------------------------------------------------
# 5. kernel selection
# ------------------------------------------------------------------------------------------------
def test_valu_rollout_is_refused_and_default_is_persistent():
    E, T = 37, 48
    cfg = ppo_amd.ACPPOConfig(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=1, update_epochs=1,
                              total_timesteps=E * T * 2)
    tr = ppo_amd.Trainer(cfg, options="rollout_kernel=valu")
    try:
        with pytest.raises(ppo_amd.PPOError, match=r"rollout_kernel=valu.*PSYN_QUADROTOR"):
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
    # E = 37 <= 512: the synthetic cheetah would take k_rollout_v here; this kind takes k_rollout
    _assert_rollout_pair_equal(cfg, [None, "rollout=per_step"], T2=5)


# ------------------------------------------------------------------------------------------------
# 6. one iteration against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_one_iteration_vs_oracle(kind):
    """One iteration (E = 37, T = 16, one minibatch, one epoch) at O = 18, A = 4 against the oracle with
    the bars of test_gpu_reacher.py::test_one_iteration_vs_oracle: teacher-forced act per stored step
    (A = 4: the summed log-probability), GAE bit-exact, loss statistics (the summed entropy among them)
    and parameters after one Adam step. The envs first take 40 per-step env steps with the actions of
    the desynchronised run, so the 16 stored steps hold dones that differ across envs."""
    E, T, H = 37, 16, (64 if kind == 0 else 256)
    C = ppo_amd.PPOConfig if kind == 0 else ppo_amd.ACPPOConfig
    cfg = C(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=1, update_epochs=1, total_timesteps=E * T * 4, seed=3)
    L = O.layout_init(kind, OD, AD, H)
    tr = ppo_amd.Trainer(cfg)
    try:
        p0 = tr.agent.params().copy()
        assert p0.size == L.P
        _feed(tr, qc.gpu_actions()[:40])
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
    alld = np.concatenate([g["dones"], g["next_done"][None]])
    per_step = alld.sum(1)
    print(f"dones per step {per_step.tolist()}")
    assert alld.sum() >= 3 and ((per_step > 0) & (per_step < E)).any() and (alld.sum(0) > 0).sum() >= 3
    assert len({tuple(alld[:, e].tolist()) for e in range(E)}) >= 3  # dones that differ across envs
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
# 7. CLIs
# ------------------------------------------------------------------------------------------------
def _run(args, timeout=240):
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("exe,kind,H", [("ac_ppo_continuous_action", ppo_amd.PPO_NET_LN_BETA, 256),
                                        ("ppo_continuous_action", ppo_amd.PPO_NET_TANH_NORMAL, 64)])
def test_cli_host_equals_device_env(exe, kind, H):
    """--env_id QuadrotorHover-v0 with host envs (gymcpp::QuadrotorHover; the PPO trainer's behind the
    wrapper chain) and with the device env: bit-identical final weights after two iterations of E = 8
    envs x 64 steps."""
    E, T = 8, 64
    common = ["--env_id", ENV, "--num_envs", str(E), "--num_steps", str(T), "--total_timesteps", str(E * T * 2),
              "--seed", "4", "--num_eval_runs", "2"]
    path = os.path.join(PKG, "bin", exe)
    outs = {}
    for backend in ("host", "device"):
        outs[backend] = _run([path, "--env_backend", backend, "--exp_name_stem", f"t_quad_{exe[:2]}_{backend}"] + common)
        assert "Average evaluation return=" in outs[backend]
    L = ppo_amd.agent_layout(kind, OD, AD, H)
    a = ppo_amd.load_agent_pth(L, os.path.join(MODELS, f"t_quad_{exe[:2]}_host_4", "model_final.pth"))
    b = ppo_amd.load_agent_pth(L, os.path.join(MODELS, f"t_quad_{exe[:2]}_device_4", "model_final.pth"))
    assert a.size == L.P and np.isfinite(a).all()
    np.testing.assert_array_equal(a, b)
    if exe.startswith("ac"):  # mean-action evaluation on env 0: the same episodes on both backends
        ev = {k: [ln for ln in v.splitlines() if ln.startswith("Evaluation result")] for k, v in outs.items()}
        assert len(ev["host"]) == 2 and ev["host"] == ev["device"]


# ------------------------------------------------------------------------------------------------
# 8. it learns
# ------------------------------------------------------------------------------------------------
def _learns(ref_name):
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "quadrotor", ref_name)))
    c = ref["config"]
    assert ref["condition_met"] and ref["env_id"] == ENV and len(ref["seeds"]) == 3
    bar = 0.5 * min(r["trained"] - r["untrained"] for r in ref["runs"])
    assert bar > 0
    C = ppo_amd.PPOConfig if c["agent"] == "ppo" else ppo_amd.ACPPOConfig
    E = c["num_envs"]
    for seed in ref["seeds"]:
        cfg = C(env_id=ENV, seed=seed, **{k: c[k] for k in ("num_envs", "num_steps", "total_timesteps", "num_minibatches",
                                                          "update_epochs", "learning_rate", "gamma", "gae_lambda", "clip_coef",
                                                          "ent_coef", "vf_coef", "max_grad_norm", "adam_eps")})
        tr = ppo_amd.Trainer(cfg)
        try:
            def evaluate():
                r, ln, _ = tr.agent.evaluate(tr.env, ref["eval_episodes"], ppo_amd.PPO_MEAN, eval_seed=c["eval_seed"],
                                             num_eval_envs=E, chunk_steps=1 if tr.wrappers is not None else 0)
                assert r.size >= ref["eval_episodes"] and (ln <= 500).all() and (r > 0).all()
                return float(r.astype(np.float64).mean())
            untrained = evaluate()
            tr.env.reset(cfg.seed, tr.next_obs, tr.next_done, ppo_amd.lib().ppo_stream(tr.agent.h))
            for _ in range(cfg.num_iterations):
                tr.iterate()
            trained = evaluate()
        finally:
            tr.close()
        print(f"{c['agent']} seed {seed}: untrained {untrained:.1f} -> trained {trained:.1f} "
              f"(improvement {trained - untrained:.1f}, bar {bar:.1f})")
        assert trained - untrained >= bar, (seed, untrained, trained, bar)


def test_it_learns():
    """ppo_amd.Trainer (the PPO agent, wrapper chain on, k_rollout4<2, 1, ., PSYN_QUADROTOR> at A = 4)
    with the config and seeds of tests/golden/quadrotor/learning_ref.json (written by
    scripts/quadrotor_learning_ref.py: the same loop on the CPU from the oracle and the host env),
    under the protocol of test_gpu_cartpole.py::test_it_learns. Per seed, the improvement of the
    mean-action evaluation return (the first 64 episodes, Agent.evaluate on all envs) from before to
    after training must be at least half the smallest improvement of the reference: the GPU and CPU
    trajectories part at the first rounding difference, so what is compared is whether learning
    happens, not a curve.
    Measured (MI355X): seeds 1, 2, 3 improve by 18.0, 20.1, 14.0; the reference by 24.0, 36.6, 22.7;
    the bar is 11.3."""
    _learns("learning_ref.json")


def test_it_learns_ac():
    """The AC agent (LayerNorm-Beta, H = 256, no wrappers; k_rollout<2, 1, PSYN_QUADROTOR>, evaluation by
    k_eval<2, 1, PSYN_QUADROTOR>) with the config and seeds of tests/golden/quadrotor/learning_ref_ac.json,
    the same script's run with --agent ac, and the same bar.
    Measured (MI355X): seeds 1, 2, 3 improve by 53.4, 40.0, 32.5; the reference by 43.1, 33.8, 16.5;
    the bar is 8.3."""
    _learns("learning_ref_ac.json")
