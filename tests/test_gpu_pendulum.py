"""Pendulum-v1 on the device (env kind PSYN_PENDULUM, include/ppo_synth_env.h) through the C-ABI.

  1. the per-step device env (k_env_reset<PSYN_PENDULUM> / k_env_step<PSYN_PENDULUM>) is the host env gymcpp/pendulum.h bit for
     bit, without and with the PPO wrapper chain;
  2. the persistent rollouts (k_rollout, k_rollout4 at 4 and at 16 envs per workgroup) are the
     per-step path bit for bit;
  3. the persistent evaluation (k_eval) is the per-step evaluation bit for bit;
  4. rollout_kernel=valu is refused for this env kind; the default options take the persistent path;
  5. an agent with obs_dim 3 / act_dim 1 against the CPU oracle: act, GAE, one update;
  6. both CLIs train Pendulum-v1 with host envs and with the device env to the same weights;
  7. the trainer learns the task (bar from the CPU reference run, tests/golden/pendulum).
"""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ppo.cpp_amd")
MODELS = os.path.join(PKG, "models")
ENV = "Pendulum-v1"
OD, AD = 3, 1


# ------------------------------------------------------------------------------------------------
# 1. device per-step env == host env
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pend") / "pendulum_driver")
    subprocess.run(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-pthread",
                    os.path.join(ROOT, "tests", "native", "pendulum_driver.cpp"), "-o", exe], check=True)
    return exe


def _host_run(driver, tmp_path, E, T, seed, act, wrapped):
    act.tofile(tmp_path / "a.f32")
    args = [driver, "vecw" if wrapped else "vec", str(E), str(T), str(seed), "1", str(tmp_path / "a.f32"),
            str(tmp_path / "o.f32")] + (["0.99"] if wrapped else [])
    subprocess.run(args, check=True)
    out = np.fromfile(tmp_path / "o.f32", np.float32)
    per = E * OD + 5 * E
    s = out[E * OD:].reshape(T, per)
    return out[:E * OD].reshape(E, OD), {
        "obs": s[:, :E * OD].reshape(T, E, OD), "rew": s[:, E * OD:E * OD + E],
        "done": np.maximum(s[:, E * OD + E:E * OD + 2 * E], s[:, E * OD + 2 * E:E * OD + 3 * E]),
        "ret": s[:, E * OD + 3 * E:E * OD + 4 * E], "len": s[:, E * OD + 4 * E:]}


@pytest.mark.parametrize("wrapped", [False, True])
def test_device_env_bitwise_equals_host_env(driver, tmp_path, wrapped):
    """E = 37 (a ragged last block), T = 450 (two truncations with their autoresets), actions beyond
    the action space. Without wrappers everything is bitwise; with the PPO chain attached the bars are
    test_gpu_wrappers.py's: normalised observations within 1 ulp, everything else bitwise."""
    E, T, seed = 37, 450, 6
    act = np.random.default_rng(8).uniform(-3, 3, (T, E, AD)).astype(np.float32)
    h0, h = _host_run(driver, tmp_path, E, T, seed, act, wrapped)
    env = ppo_amd.SynthEnv(E, env_id=ENV)
    assert env.info() == (ppo_amd.PSYN_PENDULUM, OD, AD, 200) and (env.O, env.A) == (OD, AD)
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
        env.step(DeviceArray.from_numpy(act[t]), obs, rew, done, lo=-2.0, hi=2.0)
        same_obs(obs.numpy(), h["obs"][t], f"obs, step {t}")
        np.testing.assert_array_equal(rew.numpy().view(np.uint32), h["rew"][t].view(np.uint32), err_msg=f"reward, step {t}")
        np.testing.assert_array_equal(done.numpy(), h["done"][t], err_msg=f"done, step {t}")
        fin = h["len"][t] > 0
        fin_ret[fin] = (fin_ret[fin] + h["ret"][t][fin]).astype(np.float32)
        fin_len[fin] += h["len"][t][fin]
        fin_cnt += fin.sum()
    assert fin_cnt == 2 * E and h["done"].sum() == 2 * E
    sr, sl, n = env.episode_stats()
    assert (np.float32(sr), sl, n) == (np.float32(fin_ret.astype(np.float64).sum()), fin_len.sum(), fin_cnt)
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
    # the env state the rollouts left behind (theta, thetadot, step count, reset count): one more
    # env step from it, with the same actions, gives the same bits
    E = trs[0].hcfg.num_envs
    a = DeviceArray.from_numpy(np.linspace(-2.5, 2.5, E, dtype=np.float32).reshape(E, 1))
    outs = []
    for tr in trs:
        rew = DeviceArray(E)
        tr.env.step(a, tr.next_obs, rew, tr.next_done, lo=-2.0, hi=2.0)
        outs.append((tr.next_obs.numpy(), rew.numpy(), tr.next_done.numpy()))
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    if trs[0].wrappers is not None:
        for k, v in trs[0].wrappers.state().items():
            np.testing.assert_array_equal(v, trs[1].wrappers.state()[k], err_msg=k)
    return snaps[0]


@pytest.mark.parametrize("agent,shape", [("ac", "E37"), ("ppo", "E37"), ("ppo", "4CU+5")])
def test_persistent_rollout_bitwise_equals_per_step(agent, shape):
    """AC agent: k_rollout<1, 1, PSYN_PENDULUM> + k_values vs k_act3 + k_env_step<PSYN_PENDULUM>. PPO agent with the
    wrapper chain: k_rollout4 at 4 envs per workgroup (E = 37) and at 16 (E = 4 CUs + 5: more 4-env
    workgroups than CUs) vs k_act4 + k_env_step<PSYN_PENDULUM>. T = 210 twice crosses both truncations (steps 200,
    401) and starts the second rollout mid-episode."""
    E, T, iters = (37, 210, 2) if shape == "E37" else (4 * _cu_count() + 5, 8, 2)
    C = ppo_amd.ACPPOConfig if agent == "ac" else ppo_amd.PPOConfig
    cfg = C(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=2, update_epochs=1, total_timesteps=E * T * iters)
    trs = [ppo_amd.Trainer(cfg, options="act_kernel=4"), ppo_amd.Trainer(cfg, options="act_kernel=4,rollout=per_step")]
    try:
        assert trs[0].env.info()[0] == ppo_amd.PSYN_PENDULUM
        assert (trs[0].wrappers is not None) == (agent == "ppo")
        s = _assert_rollouts_equal(trs, iters)
        assert np.isfinite(s["values"]).all() and np.isfinite(s["logp"]).all()
        if shape == "E37":
            assert s["dones"].sum() == E  # the second rollout holds the truncation of step 401
        if agent == "ac":
            assert np.abs(s["actions"]).max() <= 2.0 and np.abs(s["actions"]).max() > 1.0
            np.testing.assert_allclose(np.hypot(s["obs"][..., 0], s["obs"][..., 1]), 1.0, atol=1e-6)
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


@pytest.mark.parametrize("name,mode", [("mean", ppo_amd.PPO_MEAN), ("roach", ppo_amd.PPO_ROACH), ("sample", ppo_amd.PPO_SAMPLE)])
@pytest.mark.parametrize("nE", [1, 19])
def test_eval_kernel_bitwise_equals_per_step(ac_agent, name, mode, nE):
    E, runs = 19, 5
    env = ppo_amd.SynthEnv(E, env_id=ENV)
    step0 = (1 << 40) if name == "sample" else 0
    fast = ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0)
    assert ac_agent.eval_info() == "eval=k_eval"
    slow = ac_agent.evaluate(env, runs, mode, eval_seed=2, num_eval_envs=nE, step0=step0, per_step=True)
    assert ac_agent.eval_info() == "eval=per_step"
    env.close()
    np.testing.assert_array_equal(fast[0].view(np.uint32), slow[0].view(np.uint32))
    np.testing.assert_array_equal(fast[1], slow[1])
    assert fast[2] == slow[2]
    assert fast[0].size == (runs if nE == 1 else nE) and (fast[1] == 200).all()
    assert fast[2] == (5 * 201 - 1 if nE == 1 else 200)
    assert np.isfinite(fast[0]).all() and (fast[0] < 0).all() and (fast[0] > -200 * 16.3).all()


# ------------------------------------------------------------------------------------------------
# 4. kernel selection
# ------------------------------------------------------------------------------------------------
def test_valu_rollout_is_refused_and_default_is_persistent():
    E, T = 64, 32
    cfg = ppo_amd.ACPPOConfig(env_id=ENV, num_envs=E, num_steps=T, num_minibatches=2, update_epochs=1,
                              total_timesteps=E * T * 2)
    tr = ppo_amd.Trainer(cfg, options="rollout_kernel=valu")
    try:
        with pytest.raises(ppo_amd.PPOError, match=r"rollout_kernel=valu.*PSYN_PENDULUM"):
            tr.rollout()
    finally:
        tr.close()
    # E = 64 <= 512: the synthetic cheetah would take k_rollout_v here; Pendulum takes k_rollout
    trs = [ppo_amd.Trainer(cfg), ppo_amd.Trainer(cfg, options="rollout=per_step")]
    try:
        _assert_rollouts_equal(trs, 1)
    finally:
        for tr in trs:
            tr.close()


# ------------------------------------------------------------------------------------------------
# 5. obs_dim 3 / act_dim 1 against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_one_iteration_vs_oracle_at_A1(kind):
    """One Pendulum iteration (E = 32, T = 16, one minibatch, one epoch) against the oracle with the
    tolerances tests/test_gpu_parity.py states for the same quantities: teacher-forced act per stored
    step (test_trainer_iteration_vs_oracle_at_metric_size), GAE bit-exact
    (test_gae_full_size_bit_exact_vs_oracle), loss statistics and parameters after one Adam step
    (test_update_vs_golden)."""
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
    """--env_id Pendulum-v1 with host envs (gymcpp::Pendulum; the PPO trainer's behind the wrapper
    chain) and with the device env: bit-identical final weights, the bar of
    test_ac_cli_host_equals_device_env / test_ppo_cli_host_equals_device_env. Two iterations of 200
    steps: the second starts with every env's autoreset."""
    E, T = 8, 200
    common = ["--env_id", ENV, "--num_envs", str(E), "--num_steps", str(T), "--total_timesteps", str(E * T * 2),
              "--seed", "4", "--num_eval_runs", "2"]
    path = os.path.join(PKG, "bin", exe)
    outs = {}
    for backend in ("host", "device"):
        outs[backend] = _run([path, "--env_backend", backend, "--exp_name_stem", f"t_pend_{exe[:2]}_{backend}"] + common)
        assert "Average evaluation return=" in outs[backend]
    L = ppo_amd.agent_layout(kind, OD, AD, H)
    a = ppo_amd.load_agent_pth(L, os.path.join(MODELS, f"t_pend_{exe[:2]}_host_4", "model_final.pth"))
    b = ppo_amd.load_agent_pth(L, os.path.join(MODELS, f"t_pend_{exe[:2]}_device_4", "model_final.pth"))
    assert a.size == L.P and np.isfinite(a).all()
    np.testing.assert_array_equal(a, b)
    if exe.startswith("ac"):  # mean-action evaluation on env 0: the same episodes on both backends
        ev = {k: [ln for ln in v.splitlines() if ln.startswith("Evaluation result")] for k, v in outs.items()}
        assert len(ev["host"]) == 2 and ev["host"] == ev["device"]


def test_cli_unknown_env_lists_pendulum():
    for exe in ("ac_ppo_continuous_action", "ppo_continuous_action"):
        r = subprocess.run([os.path.join(PKG, "bin", exe), "--env_id", "Walker2d-v5", "--env_backend", "device",
                            "--exp_name_stem", "t_pend_unknown"], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "unknown env_id Walker2d-v5" in r.stderr and "Pendulum-v1" in r.stderr


# ------------------------------------------------------------------------------------------------
# 7. it learns
# ------------------------------------------------------------------------------------------------
def test_it_learns():
    """ppo_amd.Trainer on Pendulum-v1 with the config and seeds of tests/golden/pendulum/learning_ref.json
    (written by scripts/pendulum_learning_ref.py: the same loop on the CPU from the oracle and the host
    env). Per seed, the improvement of the mean-action evaluation return (64 episodes, Agent.evaluate)
    from before to after training must be at least half the smallest improvement of the reference: the
    GPU and CPU trajectories part at the first rounding difference, so what is compared is whether
    learning happens, not a curve. The evaluation runs as one 200-step chunk, the reference's protocol (the
    per-step evaluation path runs whole chunks, and the training envs' normalisers see every step of it).
    Measured (MI355X): seeds 1, 2, 3 improve by 527.9, 516.4, 465.4; the reference by 571.9, 530.9, 496.9;
    the bar is 248.4."""
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "pendulum", "learning_ref.json")))
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
                                             num_eval_envs=E, chunk_steps=200)  # one 200-step episode per env
                assert r.size >= ref["eval_episodes"] and (ln == 200).all()
                return float(r.astype(np.float64).mean())
            untrained = evaluate()
            tr.env.reset(cfg.seed, tr.next_obs, tr.next_done, ppo_amd.lib().ppo_stream(tr.agent.h))
            for _ in range(cfg.num_iterations):
                tr.iterate()
            trained = evaluate()
        finally:
            tr.close()
        print(f"seed {seed}: untrained {untrained:.1f} -> trained {trained:.1f} (improvement {trained - untrained:.1f}, "
              f"bar {bar:.1f})")
        assert trained - untrained >= bar, (seed, untrained, trained, bar)
