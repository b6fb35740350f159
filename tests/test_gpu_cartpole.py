"""CartPoleContinuous-v1 on the device (env kind PSYN_CARTPOLE, include/ppo_synth_env.h) through the
C-ABI: the first device env whose episodes terminate, so episodes end on different steps in different
envs and the termination flag reaches NormalizeReward.

  1. the per-step device env (k_env_reset<PSYN_CARTPOLE> / k_env_step<PSYN_CARTPOLE>) is the host env gymcpp/cartpole.h bit for
     bit, without and with the PPO wrapper chain (with it: fails on a kernel that passes te = 0);
  2. the persistent rollouts (k_rollout, k_rollout4 at 4 and at 16 envs per workgroup) are the
     per-step path bit for bit;
  3. the persistent evaluation (k_eval) is the per-step evaluation bit for bit, and both are the
     event list a step-by-step replay through the public calls gives;
  4. rollout_kernel=valu is refused for this env kind; the default options take the persistent path;
  5. one iteration of both agents against the CPU oracle, GAE bit-exact on dones that differ across envs;
  6. both CLIs train the task with host envs and with the device env to the same weights;
  7. the trainer learns the task, with the PPO agent and with the AC agent (bars from the CPU
     reference runs, tests/golden/cartpole).
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cartpole_common as cc
import oracle_lib as O

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

ROOT = cc.ROOT
PKG = os.path.join(ROOT, "ppo.cpp_amd")
MODELS = os.path.join(PKG, "models")
ENV, OD, AD = cc.ENV_ID, cc.OD, cc.AD


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return cc.build_driver(str(tmp_path_factory.mktemp("cart") / "cartpole_driver"))


# ------------------------------------------------------------------------------------------------
# 1. device per-step env == host env
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrapped", [False, True])
def test_device_env_bitwise_equals_host_env(driver, tmp_path, wrapped):
    """The inputs of the desynchronisation condition (E = 37: a ragged last block; T = 450; seed 6;
    actions in [-3, 3], beyond the action space). Without wrappers everything is bitwise; with the PPO
    chain at gamma = 0.99 the normalised observations are within 1 ulp and rewards, dones, episode
    statistics and the wrapper state's reward side are bitwise (test_gpu_wrappers.py's bars). With te
    forced to 0 in k_env_step<PSYN_CARTPOLE> the wrapped case fails at the first step after a termination: the return
    accumulator keeps the finished episode's return."""
    E, T, seed = cc.DESYNC_E, cc.DESYNC_T, cc.DESYNC_SEED
    act = cc.desync_actions()
    _, h0, h = cc.host_vec(driver, tmp_path, E, T, seed, "h", act, gamma=0.99 if wrapped else None)
    hdone = np.maximum(h["term"], h["trunc"])
    cc.assert_desynchronised(hdone)
    assert h["term"].sum() > 5 * E
    env = ppo_amd.SynthEnv(E, env_id=ENV)
    assert env.info() == (ppo_amd.PSYN_CARTPOLE, OD, AD, 500) and (env.O, env.A) == (OD, AD)
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
    assert fin_cnt == hdone.sum() and fin_cnt > 5 * E
    sr, sl, n = env.episode_stats()
    assert (np.float32(sr), sl, n) == (np.float32(fin_ret.astype(np.float64).sum()), fin_len.sum(), fin_cnt)
    assert sr == sl  # reward 1 per step: return = length
    if w is not None:
        # the wrapper state after the 450 steps against the oracle's vector chain fed the host env's
        # raw stream (the unwrapped run of the same inputs) with its termination flags: every word
        # bitwise, test_gpu_wrappers.py's bar. rew_acc is the word a te = 0 kernel gets wrong.
        _, r0, raw = cc.host_vec(driver, tmp_path, E, T, seed, "raw", act)
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
        # the final step itself holds terminations (3 on the host), which no later reward would
        # show; the envs stand at different points of their episodes, so their accumulators differ
        assert raw["term"][T - 1].any() and not raw["term"][T - 1].all()
        assert len(set(st["rew_acc"].tolist())) > E // 2
    env.close()
    if w is not None:
        w.close()


# ------------------------------------------------------------------------------------------------
# 2. persistent rollout == per-step rollout
# ------------------------------------------------------------------------------------------------
BUFS = [("obs", "BUF_OBS", 1), ("actions", "BUF_ACTIONS", 2), ("logp", "BUF_LOGPROBS", 0),
        ("rewards", "BUF_REWARDS", 0), ("dones", "BUF_DONES", 0), ("values", "BUF_VALUES", 0)]


def snapshot(tr):
    E, T, O_, A = tr.hcfg.num_envs, tr.hcfg.num_steps, tr.hcfg.obs_dim, tr.hcfg.act_dim
    out = {}
    for name, b, kind in BUFS:
        shape = (T, E, O_) if kind == 1 else (T, E, A) if kind == 2 else (T, E)
        out[name] = tr.agent.buffer(getattr(ppo_amd, b), shape).numpy()
    out["next_obs"] = tr.next_obs.numpy()
    out["next_done"] = tr.next_done.numpy()
    return out


def _cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _advance(tr, steps, seed=21):
    """`steps` per-step env steps (k_env_step<PSYN_CARTPOLE>, through the wrapper chain where attached) with actions
    uniform in [-3, 3], into the trainer's next_obs / next_done: the envs are then spread over their
    episodes (lengths 9 .. 71 under such actions), so a short rollout meets terminations."""
    E = tr.hcfg.num_envs
    act = np.random.default_rng(seed).uniform(-3, 3, (steps, E, AD)).astype(np.float32)
    rew = DeviceArray(E)
    for t in range(steps):
        tr.env.step(DeviceArray.from_numpy(act[t]), tr.next_obs, rew, tr.next_done, lo=-1.0, hi=1.0)
    rew.numpy()  # a blocking copy: the steps have run before the rollout starts on the agent's stream
    tr.agent.sync()


def _assert_rollouts_equal(trs, iters):
    all_dones = []
    for it in range(iters):
        snaps, stats = [], []
        for tr in trs:
            tr.rollout()
            tr.agent.sync()
            snaps.append(snapshot(tr))
            stats.append(tr.env.episode_stats())
            tr.agent.compute_gae(tr.next_obs, tr.next_done)
            tr.agent.update(tr.lr_now(), want_stats=False)
            tr.iteration += 1
        for k in snaps[0]:
            np.testing.assert_array_equal(snaps[0][k].view(np.uint32), snaps[1][k].view(np.uint32),
                                          err_msg=f"iteration {it}: {k}")
        assert stats[0] == stats[1], it
        np.testing.assert_array_equal(trs[0].agent.params(), trs[1].agent.params(), err_msg=f"iteration {it}")
        all_dones.append(snaps[0]["dones"])
    # the env state the rollouts left behind (x, xdot, theta, thetadot, step count, reset count,
    # autoreset flag): one more env step from it, with the same actions, gives the same bits
    E = trs[0].hcfg.num_envs
    a = DeviceArray.from_numpy(np.linspace(-1.5, 1.5, E, dtype=np.float32).reshape(E, 1))
    outs = []
    for tr in trs:
        rew = DeviceArray(E)
        tr.env.step(a, tr.next_obs, rew, tr.next_done, lo=-1.0, hi=1.0)
        outs.append((tr.next_obs.numpy(), rew.numpy(), tr.next_done.numpy()))
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    if trs[0].wrappers is not None:
        for k, v in trs[0].wrappers.state().items():
            np.testing.assert_array_equal(v, trs[1].wrappers.state()[k], err_msg=k)
    return snaps[0], np.concatenate(all_dones)


@pytest.mark.parametrize("agent,shape", [("ac", "E37"), ("ppo", "E37"), ("ppo", "4CU+5")])
def test_persistent_rollout_bitwise_equals_per_step(agent, shape):
    """AC agent: k_rollout<1, 1, PSYN_CARTPOLE> + k_values vs k_act3 + k_env_step<PSYN_CARTPOLE>. PPO agent with the
    wrapper chain: k_rollout4 at 4 envs per workgroup (E = 37) and at 16 (E = 4 CUs + 5: more 4-env
    workgroups than CUs) vs k_act4 + k_env_step<PSYN_CARTPOLE>. Compared: all storage buffers, next_obs / next_done,
    the env state (one more step from it), the wrapper state, the episode statistics and the parameters
    after each update. E = 37, T = 210, 2 iterations: every env finishes several episodes, on its own
    steps, and dones.sum() > E. E = 4 CUs + 5, T = 8, 12 iterations: 96 steps, in which the sampled
    policy's episodes (some 20 steps long) end several times in every env, each rollout starting
    mid-episode; dones.sum() > E there as well, and single envs of a 16-env workgroup finish alone."""
    big = shape != "E37"
    E, T, iters = (4 * _cu_count() + 5, 8, 12) if big else (37, 210, 2)
    C = ppo_amd.ACPPOConfig if agent == "ac" else ppo_amd.PPOConfig
    cfg = C(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=2, update_epochs=1, total_timesteps=E * T * iters)
    trs = [ppo_amd.Trainer(cfg, options="act_kernel=4"), ppo_amd.Trainer(cfg, options="act_kernel=4,rollout=per_step")]
    try:
        assert trs[0].env.info()[0] == ppo_amd.PSYN_CARTPOLE
        assert (trs[0].wrappers is not None) == (agent == "ppo")
        s, dones = _assert_rollouts_equal(trs, iters)
        assert np.isfinite(s["values"]).all() and np.isfinite(s["logp"]).all()
        per_step = dones.sum(1)
        print(f"{agent} {shape}: {int(dones.sum())} dones in {len(dones)} steps of {E} envs, on {int((per_step > 0).sum())} steps")
        assert ((per_step > 0) & (per_step < E)).any()  # the dones of one step are not all equal
        if big:
            assert dones.sum() > E and (per_step > 0).sum() >= 8
            blk = dones[:, :16 * (E // 16)].reshape(len(dones), -1, 16).sum(2)
            assert (blk == 1).any()  # one env of a 16-env workgroup finishes, its neighbours do not
        else:
            assert dones.sum() > E and (dones.sum(0) >= 2).all()
            blk = dones[:, :36].reshape(len(dones), 9, 4).sum(2)
            assert (blk == 1).any()  # one env of a 4-env workgroup finishes, its neighbours do not
        if agent == "ac":
            assert np.abs(s["actions"]).max() <= 1.0
    finally:
        for tr in trs:
            tr.close()


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
    psyn_step, and one event (step, env, length) per done; stops after the step at which the event
    count reaches `runs`, keeping all events of that step, in (step, env) order."""
    obs, done, rew = DeviceArray((E, OD)), DeviceArray(E), DeviceArray(E)
    env.reset(eval_seed, obs, done)
    x = DeviceArray.wrap(obs.ptr, (nE, OD))
    events, length, fresh, k = [], np.zeros(nE, np.int64), np.zeros(nE, bool), 0
    while len(events) < runs:
        act, _, _, _ = agent.get_action_and_value(x, mode, step_id=step0 + k)
        env.step(act, obs, rew, done, lo=-1.0, hi=1.0, e0=0, e1=nE)
        d = done.numpy()[:nE] != 0
        length = np.where(fresh, 0, length + 1)  # the step after a done is the reset step
        events += [(k, int(e), int(length[e])) for e in np.nonzero(d)[0]]
        fresh = d
        k += 1
        assert k < 5000
    return events, k


@pytest.mark.parametrize("name,mode", [("mean", ppo_amd.PPO_MEAN), ("roach", ppo_amd.PPO_ROACH), ("sample", ppo_amd.PPO_SAMPLE)])
@pytest.mark.parametrize("nE", [1, 19])
def test_eval_kernel_bitwise_equals_per_step(ac_agent, name, mode, nE):
    """chunk_steps = 48: several chunks (the chunk size changes no returned bit)."""
    E, runs = 19, 5
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
    print(f"{name} nE={nE}: events (step, env, length) {events}, env steps {steps}")
    # the events come in (step, env) order, and the count follows the stopping rule
    assert events == sorted(events) and fast[2] == steps
    np.testing.assert_array_equal(fast[1], [ln for _, _, ln in events])
    np.testing.assert_array_equal(fast[0], np.asarray(fast[1], np.float32))  # reward 1 per step
    assert len(set(fast[1].tolist())) > 1  # the lengths are not all equal
    assert (fast[1] >= 7).all() and (fast[1] <= 500).all()
    last = events[-1][0]
    on_last = sum(1 for k, _, _ in events if k == last)
    assert len(events) - on_last < runs <= len(events)
    if nE == 19:
        assert on_last < 19  # the rule stops on a step where fewer than all envs finish
        assert len({e for _, e, _ in events}) > 1


# ------------------------------------------------------------------------------------------------
# 4. kernel selection
# ------------------------------------------------------------------------------------------------
def test_valu_rollout_is_refused_and_default_is_persistent():
    E, T = 64, 48
    cfg = ppo_amd.ACPPOConfig(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=2, update_epochs=1,
                              total_timesteps=E * T * 2)
    tr = ppo_amd.Trainer(cfg, options="rollout_kernel=valu")
    try:
        with pytest.raises(ppo_amd.PPOError, match=r"rollout_kernel=valu.*PSYN_CARTPOLE"):
            tr.rollout()
    finally:
        tr.close()
    # E = 64 <= 512: the synthetic cheetah would take k_rollout_v here; this kind takes k_rollout
    trs = [ppo_amd.Trainer(cfg), ppo_amd.Trainer(cfg, options="rollout=per_step")]
    try:
        _, dones = _assert_rollouts_equal(trs, 1)
        assert dones.sum() > 0
    finally:
        for tr in trs:
            tr.close()


# ------------------------------------------------------------------------------------------------
# 5. one iteration against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_one_iteration_vs_oracle(kind):
    """One iteration (E = 32, T = 16, one minibatch, one epoch) against the oracle with the bars of
    test_gpu_pendulum.py::test_one_iteration_vs_oracle_at_A1: teacher-forced act per stored step, GAE
    bit-exact, loss statistics and parameters after one Adam step. The envs first take 24 per-step env
    steps (actions in [-3, 3]), so the 16 stored steps hold dones that differ across envs."""
    E, T, H = 32, 16, (64 if kind == 0 else 256)
    C = ppo_amd.PPOConfig if kind == 0 else ppo_amd.ACPPOConfig
    cfg = C(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=1, update_epochs=1, total_timesteps=E * T * 4, seed=3)
    L = O.layout_init(kind, OD, AD, H)
    tr = ppo_amd.Trainer(cfg)
    try:
        p0 = tr.agent.params().copy()
        assert p0.size == L.P
        _advance(tr, 24)
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
# 6. CLIs
# ------------------------------------------------------------------------------------------------
def _run(args, timeout=240):
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("exe,kind,H", [("ac_ppo_continuous_action", ppo_amd.PPO_NET_LN_BETA, 256),
                                        ("ppo_continuous_action", ppo_amd.PPO_NET_TANH_NORMAL, 64)])
def test_cli_host_equals_device_env(exe, kind, H):
    """--env_id CartPoleContinuous-v1 with host envs (gymcpp::CartPoleContinuous; the PPO trainer's
    behind the wrapper chain) and with the device env: bit-identical final weights after two
    iterations of E = 64 envs x 64 steps. Both runs report finished training episodes with returns
    below 500: episodes that terminated (reward 1 per step, truncation only at 500), inside the rollouts."""
    E, T = 64, 64
    common = ["--env_id", ENV, "--num_envs", str(E), "--num_steps", str(T), "--total_timesteps", str(E * T * 2),
              "--seed", "4", "--num_eval_runs", "2"]
    path = os.path.join(PKG, "bin", exe)
    outs = {}
    for backend in ("host", "device"):
        outs[backend] = _run([path, "--env_backend", backend, "--exp_name_stem", f"t_cart_{exe[:2]}_{backend}"] + common)
        assert "Average evaluation return=" in outs[backend]
        ep = [float(x) for x in re.findall(r"^global_step=\d+, (?:avg_)?episodic_return=([0-9.]+)", outs[backend], re.M)]
        assert ep and 7 <= min(ep) and max(ep) < 500, ep[:5]
    L = ppo_amd.agent_layout(kind, OD, AD, H)
    a = ppo_amd.load_agent_pth(L, os.path.join(MODELS, f"t_cart_{exe[:2]}_host_4", "model_final.pth"))
    b = ppo_amd.load_agent_pth(L, os.path.join(MODELS, f"t_cart_{exe[:2]}_device_4", "model_final.pth"))
    assert a.size == L.P and np.isfinite(a).all()
    np.testing.assert_array_equal(a, b)
    if exe.startswith("ac"):  # mean-action evaluation on env 0: the same episodes on both backends
        ev = {k: [ln for ln in v.splitlines() if ln.startswith("Evaluation result")] for k, v in outs.items()}
        assert len(ev["host"]) == 2 and ev["host"] == ev["device"]


def test_cli_unknown_env_lists_cartpole():
    for exe in ("ac_ppo_continuous_action", "ppo_continuous_action"):
        r = subprocess.run([os.path.join(PKG, "bin", exe), "--env_id", "Walker2d-v5", "--env_backend", "device",
                            "--exp_name_stem", "t_cart_unknown"], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "unknown env_id Walker2d-v5" in r.stderr and ENV in r.stderr


# ------------------------------------------------------------------------------------------------
# 7. it learns
# ------------------------------------------------------------------------------------------------
def _learns(ref_name):
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "cartpole", ref_name)))
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
                assert r.size >= ref["eval_episodes"] and (r == ln).all()
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
    """ppo_amd.Trainer (the PPO agent, wrapper chain on) with the config and seeds of
    tests/golden/cartpole/learning_ref.json (written by scripts/cartpole_learning_ref.py: the same loop
    on the CPU from the oracle and the host env). Per seed, the improvement of the mean-action
    evaluation return (64 episodes, Agent.evaluate on all envs) from before to after training must be
    at least half the smallest improvement of the reference: the GPU and CPU trajectories part at the
    first rounding difference, so what is compared is whether learning happens, not a curve. The
    evaluation runs in chunks of one step, the reference's protocol: it stops on the step at which the
    64th episode ends, and the training envs' normalisers see exactly those steps.
    Measured (MI355X): seeds 1, 2, 3 improve by 116.3, 106.1, 99.6; the reference by 114.5, 102.5, 101.4;
    the bar is 50.7."""
    _learns("learning_ref.json")


def test_it_learns_ac():
    """The AC agent (LayerNorm-Beta, H = 256, no wrappers; k_rollout<1, 1, PSYN_CARTPOLE>) with the config
    and seeds of tests/golden/cartpole/learning_ref_ac.json, the same script's run with --agent ac, and
    the same bar: half the smallest improvement of the reference. Its evaluation is k_eval.
    Measured (MI355X): seeds 1, 2, 3 improve by 266.4, 131.1, 435.0; the reference by 218.1, 415.9, 190.4;
    the bar is 95.2."""
    _learns("learning_ref_ac.json")
