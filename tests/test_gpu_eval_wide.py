"""k_eval_w (csrc/ppo_eval_wide.hip): the AC agent's persistent evaluation kernel at Humanoid width
(LayerNorm-Beta, H = 256, OP = 384, 17 <= A <= 24, the cheetah-shaped env without a wrapper chain).

It runs k_act3<LN_BETA, 24, 3>'s chain and k_synth_step_wide's step, so it must return the per-step
path's bits and leave the per-step path's env state; the default takes it; against the CPU oracle it
is held to twice the per-step path's measured gap. ppo_evaluate_synth runs until the asked episodes
have finished (an episode is 1 000 steps), so the short-chunk cases run 1 008 and 1 024 steps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402
from test_gpu_eval import MODES, SEED, STEP0  # noqa: E402

_AGENTS = {}


def agent(O, A):
    """The AC agent at (O, A) on an acting-only context, shared and never modified: every parameter off its
    initial value, an obs mean / std that is not the identity."""
    if (O, A) not in _AGENTS:
        hc = ppo_amd.HipConfig(ppo_amd.PPO_NET_LN_BETA, O, A, 256, 64, 4, 1, 1, 0.99, 0.95, 0.2, 0.01, 0.5, 0.5, 1e-5, 1, 1, 1, 0, 1)
        ag = ppo_amd.Agent(hc, options="update=off")  # the default refuses A >= 13 at hidden 256: the update kernel's LDS
        rng = np.random.default_rng(4)
        p0 = ppo_amd.init_params(ag.layout, seed=3, obs_mean=0.1 * rng.standard_normal(O), obs_std=rng.uniform(0.5, 2.0, O))
        p = p0 + 0.05 * rng.standard_normal(p0.size).astype(np.float32)
        for off, n in ((ag.layout.hi, 1), (ag.layout.lo, 1), (ag.layout.omean, O), (ag.layout.ostd, O)):
            p[off:off + n] = p0[off:off + n]
        ag.load_params(p)
        _AGENTS[(O, A)] = ag
    return _AGENTS[(O, A)]


def state_after(ag, env, E):
    """The env state a call leaves, through one further step of all E envs and the episode totals."""
    obs, rew, done = DeviceArray((E, env.O)), DeviceArray(E), DeviceArray(E)
    env.step(DeviceArray.from_numpy(np.full((E, env.A), 0.1, np.float32)), obs, rew, done, stream=ppo_amd.lib().ppo_stream(ag.h))
    return {"obs": obs.numpy(), "rew": rew.numpy(), "done": done.numpy(), "totals": np.array(env.episode_stats(), np.float32)}


# id: O, A, E, nE, runs, chunk_steps, env steps to the last kept episode
CASES = {
    "one-env-chunk-333": (376, 17, 1, 1, 2, 333, 2001),     # two episodes across the autoreset
    "one-env-chunk-1001": (376, 17, 1, 1, 2, 1001, 2001),   # a launch boundary right after the autoreset step
    "ragged-o373": (373, 17, 5, 3, 3, 48, 1000),            # zero-padded input columns, 3 of 16 rows, tail envs
    "two-workgroups-a20": (376, 20, 17, 17, 17, 64, 1000),  # the widest act_dim a context takes: 640 Beta items
}


@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_persistent_bitwise_equals_per_step(case, name):
    O, A, E, nE, runs, chunk, steps = CASES[case]
    ag = agent(O, A)
    kw = dict(eval_seed=SEED, num_eval_envs=nE, chunk_steps=chunk, step0=STEP0 if name == "sample" else 0)
    out = []
    for how, info in ((dict(persistent=True), "eval=k_eval_w"), (dict(per_step=True), "eval=per_step")):
        env = ppo_amd.SynthEnv(E, O, A)
        res = ag.evaluate(env, runs, MODES[name], **kw, **how)
        assert ag.eval_info() == info
        out.append((res, state_after(ag, env, E)))
        env.close()
    (fast, fs), (slow, ss) = out
    assert fast[0].size == runs and fast[2] == steps and list(fast[1]) == [1000] * runs and np.isfinite(fast[0]).all()
    np.testing.assert_array_equal(fast[0].view(np.uint32), slow[0].view(np.uint32))
    np.testing.assert_array_equal(fast[1], slow[1])
    assert fast[2] == slow[2]
    for k in ss:
        np.testing.assert_array_equal(fs[k].view(np.uint32), ss[k].view(np.uint32), err_msg=k)
    if nE < E:  # the envs past num_eval_envs: what a reset and the one further step alone leave
        env = ppo_amd.SynthEnv(E, O, A)
        env.reset(SEED, DeviceArray((E, O)), DeviceArray(E), ppo_amd.lib().ppo_stream(ag.h))
        tail = state_after(ag, env, E)
        env.close()
        np.testing.assert_array_equal(fs["obs"][nE:].view(np.uint32), tail["obs"][nE:].view(np.uint32))


def test_the_default_takes_it_and_wrappers_do_not():
    ag = agent(376, 17)
    env = ppo_amd.SynthEnv(1, 376, 17)
    auto = ag.evaluate(env, 2, ppo_amd.PPO_MEAN)
    assert ag.eval_info() == "eval=k_eval_w" and auto[2] == 2001
    wr = ppo_amd.EnvWrappers(1, 376, 0.99)
    env.attach_wrappers(wr)
    ag.evaluate(env, 2, ppo_amd.PPO_MEAN)
    assert ag.eval_info() == "eval=per_step"
    with pytest.raises(ppo_amd.PPOError, match="wrapper chain"):
        ag.evaluate(env, 2, ppo_amd.PPO_MEAN, persistent=True)
    env.close()
    wr.close()


# max |return(device) - return(oracle)| over the two episodes, per-step path (mode = 1), measured on an
# MI355X at O = 376, A = 17: 7.629e-06 (oracle returns -41.11560822, -39.63481522: two fp32 ulps). The bound is
# 2x that figure.
PER_STEP_ORACLE_GAP = 7.629e-06


def test_eval_wide_against_the_cpu_oracle():
    """E = 1, PPO_MEAN, two episodes replayed on the CPU (orc_env_reset / orc_get_action_and_value mode 2 /
    orc_env_step), as test_gpu_eval.py's oracle test at O = 17. Both paths are held to 2x the per-step
    path's measured gap; k_eval_w measured the same 7.629e-06 (it is bitwise the per-step path)."""
    import oracle_lib as Orc
    O, A = 376, 17
    ag = agent(O, A)
    L, p = Orc.layout_init(1, O, A, 256), ag.params()
    oenv = Orc.SynthEnv(1, O, A)
    obs, orets = oenv.reset(SEED), []
    for k in range(2001):
        act, _, _, _ = Orc.get_action_and_value(L, p, obs, 2)
        obs, r, te, tr, ir, il = oenv.step(act)
        if tr[0] != 0:
            orets.append(ir[0])
    orets = np.array(orets, np.float64)
    assert orets.size == 2
    env = ppo_amd.SynthEnv(1, O, A)
    slow = ag.evaluate(env, 2, ppo_amd.PPO_MEAN, eval_seed=SEED, per_step=True)
    fast = ag.evaluate(env, 2, ppo_amd.PPO_MEAN, eval_seed=SEED, persistent=True)
    env.close()
    gs, gf = np.abs(slow[0] - orets).max(), np.abs(fast[0] - orets).max()
    print(f"oracle returns {orets}, per-step gap {gs:.3e}, persistent gap {gf:.3e}")
    assert gs <= 2 * PER_STEP_ORACLE_GAP and gf <= 2 * PER_STEP_ORACLE_GAP
