"""k_rollout_s (create option rollout_kernel=split): the AC agent's persistent rollout with 2 envs per
workgroup and the layers' k range split over wave halves, for every device env kind.
  1. teacher-forced against the fp64 oracle (the rollout part and the bars of
     test_gpu_parity.py::test_trainer_iteration_vs_oracle_at_metric_size), and run-to-run determinism;
  2. the env stepping inside the kernel is bitwise the per-step device env's, across episode ends;
  3. refusals and kernel_info.
"""
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

OPT = "rollout_kernel=split"
T = 128
BUFS = {"obs": ppo_amd.BUF_OBS, "actions": ppo_amd.BUF_ACTIONS, "logp": ppo_amd.BUF_LOGPROBS,
        "rewards": ppo_amd.BUF_REWARDS, "dones": ppo_amd.BUF_DONES}


def _rollouts(env_id, E, launches=1, seed=1, params=None):
    """`launches` consecutive rollouts of T steps: their stored buffers with next_obs / next_done, the
    parameters, the config and the env's episode statistics after the last"""
    O_, A = ppo_amd.ENV_DIMS[env_id][:2]
    cfg = ppo_amd.ACPPOConfig(env_id=env_id, num_envs=E, num_steps=T, num_minibatches=1, update_epochs=1,
                              total_timesteps=E * T * 4, seed=seed)
    tr = ppo_amd.Trainer(cfg, options=OPT, params=params)
    try:
        assert "k_rollout_s" in tr.agent.kernel_info()
        out = []
        for _ in range(launches):
            tr.rollout()
            tr.agent.sync()
            g = {k: tr.agent.buffer(b, (T, E, O_) if k == "obs" else (T, E, A) if k == "actions" else (T, E)).numpy()
                 for k, b in BUFS.items()}
            g["next_obs"], g["next_done"] = tr.next_obs.numpy(), tr.next_done.numpy()
            out.append(g)
        return out, tr.agent.params().copy(), cfg, tr.env.episode_stats()
    finally:
        tr.close()


@pytest.mark.parametrize("env_id,E", [("HalfCheetah-v5", 3), ("Hopper-v5", 2), ("Pendulum-v1", 5), ("QuadrotorHover-v0", 5)])
def test_split_rollout_teacher_forced_vs_oracle(env_id, E):
    """NTO = 2 with the cheetah's lane step and an absent second env in the last workgroup (E = 3); NTO = 1
    with an observation normalisation table (Hopper); A = 1 (Pendulum); NTO = 2, A = 4, the in-place step
    and terminations (Quadrotor). The oracle acts on the GPU's stored observations with the same Philox
    counters; a Marsaglia-Tsang acceptance flipped by a rounding may move single samples, so at most
    max(1, 1e-4 * rows) rows may lie outside. The cheetah cases also step the oracle env with the GPU's
    actions. A second run from the same seed returns the same bits (the k-halves meet in a fixed order)."""
    (g,), p0, cfg, _ = _rollouts(env_id, E)
    (g2,), _, _, _ = _rollouts(env_id, E)
    for k in g:
        np.testing.assert_array_equal(g[k].view(np.uint32), g2[k].view(np.uint32), err_msg=k)
    O_, A, lo, hi = ppo_amd.ENV_DIMS[env_id]
    L = O.layout_init(1, O_, A, 256)
    cheetah = env_id not in ppo_amd.DEVICE_ENV_KINDS
    if cheetah:
        oenv = O.SynthEnv(E, O_, A, wrappers=False, gamma=cfg.gamma)
        np.testing.assert_allclose(g["obs"][0], oenv.reset(cfg.seed), rtol=1e-5, atol=1e-6)
    else:
        assert np.abs(g["actions"]).max() <= hi and (env_id != "QuadrotorHover-v0" or g["dones"].sum() > 0)
    bad = 0
    for t in range(T):
        a, lp, _, _ = O.get_action_and_value(L, p0, g["obs"][t], 0, seed=cfg.seed, rank=0, env_base=0, step_id=t)
        close = np.isclose(g["actions"][t], a, rtol=1e-4, atol=1e-4).all(axis=1)
        close &= np.isclose(g["logp"][t], lp, rtol=1e-4, atol=1e-3)
        bad += int((~close).sum())
        if cheetah:
            nobs, r, _, _, _, _ = oenv.step(g["actions"][t], lo, hi)
            np.testing.assert_allclose(g["obs"][t + 1] if t + 1 < T else g["next_obs"], nobs, rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(g["rewards"][t], r, rtol=1e-5, atol=1e-6)
    print(f"{env_id} E={E}: rows outside {bad} of {T * E}")
    assert bad <= max(1, 1e-4 * T * E), (bad, T * E)


@pytest.mark.parametrize("env_id", ["CartPoleContinuous-v1", "QuadrotorHover-v0", "AcrobotContinuous-v1"])
def test_split_rollout_env_steps_bitwise_per_step_env(env_id):
    """Two launches of T = 128 at E = 5 (an absent env in the last workgroup); the stored actions replayed
    through the per-step device env (psyn_create_env / psyn_reset / psyn_step) from the same reset seed
    give the stored observations, rewards and dones, next_obs / next_done and the episode statistics bit
    for bit, and episodes end inside the launches (Acrobot: the swing-up parameters of its GPU tests)."""
    E, (O_, A, lo, hi) = 5, ppo_amd.ENV_DIMS[env_id]
    params = None
    if env_id == "AcrobotContinuous-v1":
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        params = np.load(os.path.join(root, "tests", "golden", "acrobot", "params_ac.npy")).astype(np.float32)
    gs, _, cfg, stats = _rollouts(env_id, E, launches=2, seed=3, params=params)
    env = ppo_amd.SynthEnv(E, env_id=env_id)
    try:
        obs, rew, done = DeviceArray((E, O_)), DeviceArray(E), DeviceArray(E)
        env.reset(cfg.seed, obs, done)
        for g in gs:
            for t in range(T):
                np.testing.assert_array_equal(g["obs"][t].view(np.uint32), obs.numpy().view(np.uint32), err_msg=f"obs {t}")
                np.testing.assert_array_equal(g["dones"][t], done.numpy(), err_msg=f"dones {t}")
                env.step(DeviceArray.from_numpy(np.ascontiguousarray(g["actions"][t])), obs, rew, done, lo=lo, hi=hi)
                np.testing.assert_array_equal(g["rewards"][t].view(np.uint32), rew.numpy().view(np.uint32), err_msg=f"rewards {t}")
            np.testing.assert_array_equal(g["next_obs"].view(np.uint32), obs.numpy().view(np.uint32))
            np.testing.assert_array_equal(g["next_done"], done.numpy())
        assert stats == env.episode_stats()
    finally:
        env.close()
    ends = sum(int(g["dones"][1:].sum() + g["next_done"].sum()) for g in gs)
    print(f"{env_id}: episodes ended inside the launches {ends}, statistics {stats}")
    assert ends >= 1 and stats[2] >= 1


def test_split_rollout_refusals():
    """The option's own refusals (not the parser's "unknown option"): at create for the tanh-Normal PPO
    agent, for O > 32 (Ant-v5) and with rollout=per_step, which would bypass the kernel; at the rollout for
    an env with the device wrapper chain, which the kernel does not run."""
    def cfg(C, env_id):
        return C(env_id=env_id, num_envs=4, num_steps=4, num_minibatches=1, update_epochs=1, total_timesteps=64)
    for C, env_id, opts, msg in ((ppo_amd.PPOConfig, "HalfCheetah-v5", OPT, "needs the LayerNorm-Beta agent"),
                                 (ppo_amd.ACPPOConfig, "Ant-v5", OPT, "needs the LayerNorm-Beta agent"),
                                 (ppo_amd.ACPPOConfig, "Pendulum-v1", OPT + ",rollout=per_step", "needs the persistent rollout")):
        with pytest.raises(ppo_amd.PPOError, match="rollout_kernel=split " + msg):
            ppo_amd.Trainer(cfg(C, env_id), options=opts)
    tr = ppo_amd.Trainer(cfg(ppo_amd.ACPPOConfig, "Pendulum-v1"), options=OPT, wrappers=True)
    try:
        with pytest.raises(ppo_amd.PPOError, match="rollout_kernel=split needs the persistent rollout"):
            tr.rollout()
    finally:
        tr.close()
