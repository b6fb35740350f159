"""AcrobotContinuous-v1 on the device (env kind PSYN_ACROBOT, include/ppo_synth_env.h) through the
C-ABI: the first device env whose step is a multi-stage integrator (RK4, four derivative evaluations
with a range reduction in front of every sine and cosine) and whose termination is success: reward -1
per step, 0 on the terminating step, and an untrained policy never terminates.

  1. the per-step device env (k_env_reset<PSYN_ACROBOT> / k_env_step<PSYN_ACROBOT>) is the host env
     gymcpp/acrobot.h bit for bit over the recorded desynchronised run, without and with the PPO
     wrapper chain;
  2. the persistent rollouts (k_rollout, k_rollout4 at 4 and at 16 envs per workgroup) are the
     per-step path bit for bit, on policies whose sampled actions swing up
     (tests/golden/acrobot/params_{ppo,ac}.npy, taken 16 iterations into the learning reference runs:
     an untrained policy would show no termination);
  3. the persistent evaluation (k_eval) is the per-step evaluation bit for bit, and both are the
     event list a step-by-step replay through the public calls gives, also with a launch boundary
     right after a terminating step and right after its autoreset step;
  4. rollout_kernel=valu is refused for this env kind; the default options take the persistent path;
  5. one iteration of both agents at O = 6, A = 1 against the CPU oracle;
  6. both CLIs train the task with host envs and with the device env to the same weights;
  7. the trainer learns the task (bars from the CPU reference runs, tests/golden/acrobot).
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import acrobot_common as ac
import oracle_lib as O

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

ROOT = ac.ROOT
PKG = os.path.join(ROOT, "ppo.cpp_amd")
MODELS = os.path.join(PKG, "models")
GOLDEN = os.path.join(ROOT, "tests", "golden", "acrobot")
ENV, OD, AD = ac.ENV_ID, ac.OD, ac.AD


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return ac.build_driver(str(tmp_path_factory.mktemp("acro") / "acrobot_driver"))


def _swing_up_params(agent):
    """Parameters of a policy whose sampled (and mean) actions swing up within some 100 to 200 steps
    (scripts/acrobot_learning_ref.py --agent AGENT --params_at 16)."""
    kind, H = (ppo_amd.PPO_NET_TANH_NORMAL, 64) if agent == "ppo" else (ppo_amd.PPO_NET_LN_BETA, 256)
    p = np.load(os.path.join(GOLDEN, f"params_{agent}.npy")).astype(np.float32)
    assert p.size == ppo_amd.agent_layout(kind, OD, AD, H).P and np.isfinite(p).all()
    return p


# ------------------------------------------------------------------------------------------------
# 1. device per-step env == host env
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrapped", [False, True])
def test_device_env_bitwise_equals_host_env(driver, tmp_path, wrapped):
    """The recorded run of the desynchronisation condition (E = 37: a ragged last block; T = 640; the
    driver's energy-pumping actions, beyond the action space). Without wrappers everything is bitwise:
    state and observation (the observation holds both speeds raw and the angles' cos / sin; one more
    step from equal observations can only be equal if the angles are), reward, done and the episode
    statistics. With the PPO chain at gamma = 0.99 the normalised observations are within 1 ulp and
    rewards, dones, episode statistics and the wrapper state are bitwise (test_gpu_wrappers.py's bars)."""
    E, T, seed = ac.DESYNC_E, ac.DESYNC_T, ac.DESYNC_SEED
    act, _, _ = ac.desync_run(driver, tmp_path)
    _, h0, h = ac.host_vec(driver, tmp_path, E, T, seed, "h", act, gamma=0.99 if wrapped else None)
    _, r0, raw = (None, h0, h) if not wrapped else ac.host_vec(driver, tmp_path, E, T, seed, "raw", act)
    counts = ac.assert_desynchronised(raw["term"], raw["trunc"])
    hdone = np.maximum(h["term"], h["trunc"])
    env = ppo_amd.SynthEnv(E, env_id=ENV)
    assert env.info() == (ppo_amd.PSYN_ACROBOT, OD, AD, 500) and (env.O, env.A) == (OD, AD)
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
    assert fin_cnt == hdone.sum() == counts["terminations"] + counts["truncations"]
    sr, sl, n = env.episode_stats()
    assert (np.float32(sr), sl, n) == (np.float32(fin_ret.astype(np.float64).sum()), fin_len.sum(), fin_cnt)
    assert sr == counts["terminations"] - sl  # -1 per step, 0 on a terminating step
    if w is not None:
        # the wrapper state after the run against the oracle's vector chain fed the host env's raw
        # stream with its termination flags: every word bitwise. rew_acc restarts after a termination
        # (not after a truncation): the word a kernel that drops the flag gets wrong.
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


def _assert_rollouts_equal(trs, iters):
    """`iters` consecutive launches (rollout, GAE, update) of both trainers: every stored buffer,
    next_obs / next_done, the episode statistics and the parameters after each update, then the env
    state the rollouts left behind (one more env step from it gives the same bits) and the wrapper
    state. Returns the last snapshot and all stored dones [iters * T, E] with next_done appended."""
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
        # dones[t] is the done flag the env raised on step t - 1: drop each launch's first row, which
        # repeats the previous launch's next_done, and append this launch's
        all_dones.append(np.concatenate([snaps[0]["dones"][1:], snaps[0]["next_done"][None]]))
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
    """AC agent: k_rollout<1, 1, PSYN_ACROBOT> + k_values vs k_act3 + k_env_step<PSYN_ACROBOT>. PPO agent with
    the wrapper chain: k_rollout4 at 4 envs per workgroup (E = 37) and at 16 (E = 4 CUs + 5: more 4-env
    workgroups than CUs) vs k_act4 + k_env_step<PSYN_ACROBOT>. Two consecutive launches each, T = 120 (E =
    37) or T = 96 (E = 4 CUs + 5), from the swing-up parameters: the sampled policies' first episodes
    end from step 77 on, each env on its own step, so both launches hold terminations at unaligned
    steps, all of them long before truncation at step 500. On the CPU (oracle act over the host env,
    the same sampling keys; no update between the launches) 240 steps of 37 envs end 47 episodes on 38
    distinct steps (PPO) and 67 on 46 (AC), 192 steps of 1 029 envs 1 008 on 94 (PPO). The thresholds
    below ask for less than half of that (at least E // 2 dones on at least 15 distinct steps, one in
    the second launch, one env finishing alone in its workgroup), since the GPU trajectories part from
    the CPU's at the first rounding difference. Measured (MI355X): 65 dones on 48 steps (AC, E = 37;
    34 in the second launch), 45 on 35 (PPO, E = 37; 29), 1 012 on 94 (PPO, E = 1 029; 973)."""
    big = shape != "E37"
    E, T, iters = (4 * _cu_count() + 5, 96, 2) if big else (37, 120, 2)
    C = ppo_amd.ACPPOConfig if agent == "ac" else ppo_amd.PPOConfig
    cfg = C(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=2, update_epochs=1, total_timesteps=E * T * iters)
    p = _swing_up_params(agent)
    trs = [ppo_amd.Trainer(cfg, options="act_kernel=4", params=p), ppo_amd.Trainer(cfg, options="act_kernel=4,rollout=per_step", params=p)]
    try:
        assert trs[0].env.info()[0] == ppo_amd.PSYN_ACROBOT
        assert (trs[0].wrappers is not None) == (agent == "ppo")
        np.testing.assert_array_equal(trs[0].agent.params(), p)
        s, dones = _assert_rollouts_equal(trs, iters)
        assert np.isfinite(s["values"]).all() and np.isfinite(s["logp"]).all()
        assert len(dones) == iters * T < 500  # every done below is a termination: no env reaches step 500
        per_step = dones.sum(1)
        second = dones[T:].sum()
        print(f"{agent} {shape}: {int(dones.sum())} dones in {len(dones)} steps of {E} envs, on {int((per_step > 0).sum())} "
              f"distinct steps; {int(second)} of them in the second launch")
        assert ((per_step > 0) & (per_step < E)).any()  # the dones of one step are not all equal
        assert dones.sum() >= E // 2 and (per_step > 0).sum() >= 15 and second >= 1
        g = 16 if big else 4
        blk = dones[:, :g * (E // g)].reshape(len(dones), -1, g).sum(2)
        assert (blk == 1).any()  # one env of a workgroup finishes, its neighbours do not
        if agent == "ac":
            assert np.abs(s["actions"]).max() <= 1.0
        # reward -1 on every step but the terminating one and the autoreset step after it (the AC agent
        # stores raw rewards; the PPO agent's are normalised)
        if agent == "ac":
            assert set(np.unique(s["rewards"]).tolist()) <= {0.0, -1.0}
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
    ag.load_params(_swing_up_params("ac"))
    yield ag
    ag.close()


def _replay_events(agent, env, E, nE, runs, mode, eval_seed, step0):
    """The evaluation through the public per-step calls: reset(eval_seed), then act on envs [0, nE),
    psyn_step, and one event (step, env, length, return) per done; stops after the step at which the
    event count reaches `runs`, keeping all events of that step, in (step, env) order."""
    obs, done, rew = DeviceArray((E, OD)), DeviceArray(E), DeviceArray(E)
    env.reset(eval_seed, obs, done)
    x = DeviceArray.wrap(obs.ptr, (nE, OD))
    events, length, ret, fresh, k = [], np.zeros(nE, np.int64), np.zeros(nE, np.float32), np.zeros(nE, bool), 0
    while len(events) < runs:
        act, _, _, _ = agent.get_action_and_value(x, mode, step_id=step0 + k)
        env.step(act, obs, rew, done, lo=-1.0, hi=1.0, e0=0, e1=nE)
        d = done.numpy()[:nE] != 0
        length = np.where(fresh, 0, length + 1)  # the step after a done is the reset step
        ret = np.where(fresh, np.float32(0), ret + rew.numpy()[:nE]).astype(np.float32)
        events += [(k, int(e), int(length[e]), float(ret[e])) for e in np.nonzero(d)[0]]
        fresh = d
        k += 1
        assert k < 5000
    return events, k


@pytest.mark.parametrize("name,mode", [("mean", ppo_amd.PPO_MEAN), ("roach", ppo_amd.PPO_ROACH), ("sample", ppo_amd.PPO_SAMPLE)])
@pytest.mark.parametrize("nE", [1, 19])
def test_eval_kernel_bitwise_equals_per_step(ac_agent, name, mode, nE):
    """E = 19 envs (a ragged workgroup), nE of them evaluated. The chunk sizes k + 1 and k + 2, k being
    the index of the first step that terminates an episode, put a launch boundary right after that
    terminating step and right after its autoreset step; 48 gives several chunks; the chunk size
    changes no returned bit."""
    E, runs = 19, 3
    env = ppo_amd.SynthEnv(E, env_id=ENV)
    step0 = (1 << 40) if name == "sample" else 0
    events, steps = _replay_events(ac_agent, env, E, nE, runs, mode, 2, step0)
    k_first = events[0][0]
    assert events[0][2] < 500  # the first episode to finish ends by termination
    fast = ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0, chunk_steps=48)
    assert ac_agent.eval_info() == "eval=k_eval"
    slow = ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0, chunk_steps=48, per_step=True)
    assert ac_agent.eval_info() == "eval=per_step"
    others = [slow, ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0)]
    for chunk in (k_first + 1, k_first + 2):
        others.append(ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0, chunk_steps=chunk))
        assert ac_agent.eval_info() == "eval=k_eval"
    env.close()
    for other in others:
        np.testing.assert_array_equal(fast[0].view(np.uint32), other[0].view(np.uint32))
        np.testing.assert_array_equal(fast[1], other[1])
        assert fast[2] == other[2]
    print(f"{name} nE={nE}: events (step, env, length, return) {events}, env steps {steps}")
    # the events come in (step, env) order, and the count follows the stopping rule
    assert events == sorted(events) and fast[2] == steps
    np.testing.assert_array_equal(fast[1], [ln for _, _, ln, _ in events])
    np.testing.assert_array_equal(fast[0], np.asarray([r for _, _, _, r in events], np.float32))
    # -1 per step, 0 on the terminating step; a truncated episode (500 steps) returns -500
    want = np.where(fast[1] < 500, 1.0 - fast[1], -500.0).astype(np.float32)
    np.testing.assert_array_equal(fast[0], want)
    assert (fast[1] >= 2).all() and (fast[1] <= 500).all() and (fast[1] < 500).any()
    last = events[-1][0]
    on_last = sum(1 for k, _, _, _ in events if k == last)
    assert len(events) - on_last < runs <= len(events)
    if nE == 19:
        assert on_last < 19  # the rule stops on a step where fewer than all envs finish
        assert len({e for _, e, _, _ in events}) > 1


# ------------------------------------------------------------------------------------------------
# 4. kernel selection
# ------------------------------------------------------------------------------------------------
def test_valu_rollout_is_refused_and_default_is_persistent():
    E, T = 64, 48
    cfg = ppo_amd.ACPPOConfig(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=2, update_epochs=1,
                              total_timesteps=E * T * 2)
    tr = ppo_amd.Trainer(cfg, options="rollout_kernel=valu")
    try:
        with pytest.raises(ppo_amd.PPOError, match=r"rollout_kernel=valu.*PSYN_ACROBOT"):
            tr.rollout()
    finally:
        tr.close()
    # E = 64 <= 512: the synthetic cheetah would take k_rollout_v here; this kind takes k_rollout
    trs = [ppo_amd.Trainer(cfg), ppo_amd.Trainer(cfg, options="rollout=per_step")]
    try:
        _assert_rollouts_equal(trs, 1)
    finally:
        for tr in trs:
            tr.close()


# ------------------------------------------------------------------------------------------------
# 5. one iteration against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_one_iteration_vs_oracle(kind):
    """One iteration (E = 32, T = 16, one minibatch, one epoch) at O = 6, A = 1 against the oracle with
    the bars of test_gpu_pendulum.py::test_one_iteration_vs_oracle_at_A1: teacher-forced act per stored
    step, GAE bit-exact, loss statistics and parameters after one Adam step."""
    E, T, H = 32, 16, (64 if kind == 0 else 256)
    C = ppo_amd.PPOConfig if kind == 0 else ppo_amd.ACPPOConfig
    cfg = C(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=1, update_epochs=1, total_timesteps=E * T * 4, seed=3)
    L = O.layout_init(kind, OD, AD, H)
    tr = ppo_amd.Trainer(cfg)
    try:
        p0 = tr.agent.params().copy()
        assert p0.size == L.P
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
    """--env_id AcrobotContinuous-v1 with host envs (gymcpp::AcrobotContinuous; the PPO trainer's
    behind the wrapper chain) and with the device env: bit-identical final weights after two
    iterations of E = 16 envs x 32 steps, and for ac_ the same evaluation episodes."""
    E, T = 16, 32
    common = ["--env_id", ENV, "--num_envs", str(E), "--num_steps", str(T), "--total_timesteps", str(E * T * 2),
              "--seed", "4", "--num_eval_runs", "2"]
    path = os.path.join(PKG, "bin", exe)
    outs = {}
    for backend in ("host", "device"):
        outs[backend] = _run([path, "--env_backend", backend, "--exp_name_stem", f"t_acro_{exe[:2]}_{backend}"] + common)
        assert "Average evaluation return=" in outs[backend]
    L = ppo_amd.agent_layout(kind, OD, AD, H)
    a = ppo_amd.load_agent_pth(L, os.path.join(MODELS, f"t_acro_{exe[:2]}_host_4", "model_final.pth"))
    b = ppo_amd.load_agent_pth(L, os.path.join(MODELS, f"t_acro_{exe[:2]}_device_4", "model_final.pth"))
    assert a.size == L.P and np.isfinite(a).all()
    np.testing.assert_array_equal(a, b)
    if exe.startswith("ac"):  # mean-action evaluation on env 0: the same episodes on both backends
        ev = {k: [ln for ln in v.splitlines() if ln.startswith("Evaluation result")] for k, v in outs.items()}
        assert len(ev["host"]) == 2 and ev["host"] == ev["device"]
        assert all(re.search(r"-500", ln) for ln in ev["host"])  # two iterations in: no swing-up yet, 500 steps at -1


def test_cli_unknown_env_lists_acrobot():
    for exe in ("ac_ppo_continuous_action", "ppo_continuous_action"):
        r = subprocess.run([os.path.join(PKG, "bin", exe), "--env_id", "Walker2d-v5", "--env_backend", "device",
                            "--exp_name_stem", "t_acro_unknown"], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "unknown env_id Walker2d-v5" in r.stderr and ENV in r.stderr


# ------------------------------------------------------------------------------------------------
# 7. it learns
# ------------------------------------------------------------------------------------------------
def _learns(ref_name):
    ref = json.load(open(os.path.join(GOLDEN, ref_name)))
    c = ref["config"]
    assert ref["condition_met"] and ref["env_id"] == ENV and len(ref["seeds"]) == 3
    bar = 0.5 * min(r["trained"] - r["untrained"] for r in ref["runs"])
    assert bar >= 25.0  # half of the 50 every reference seed had to reach
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
                assert r.size >= ref["eval_episodes"] and ((r == 1 - ln) | ((ln == 500) & (r == -500))).all()
                return float(r.astype(np.float64).mean())
            untrained = evaluate()
            assert untrained == -500.0  # the untrained mean-action policy never swings up
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
    tests/golden/acrobot/learning_ref.json (written by scripts/acrobot_learning_ref.py: the same loop
    on the CPU from the oracle and the host env). Per seed, the improvement of the mean-action
    evaluation return (64 episodes, Agent.evaluate on all envs) from before to after training must be
    at least half the smallest improvement of the reference. Every untrained return is -500, so the
    reference's own rule is an improvement of at least 50 in every seed. The evaluation runs in chunks
    of one step, the reference's protocol.
    The reference improves by 403.8, 400.1, 385.1 (seeds 1, 2, 3); the bar is 192.5. Measured (MI355X):
    -500 -> -123.3, -104.7, -124.9, improvements 376.7, 395.3, 375.1.
    There is no test_it_learns_ac: the AC agent's reference runs do not meet the rule in any config
    tried (its sampled actions never swing up), so it ships without a learning test."""
    _learns("learning_ref.json")
