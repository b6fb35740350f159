"""k_eval4 (csrc/ppo_eval4.hip): the persistent evaluation kernel of the 64-wide tanh-Normal PPO agent,
with the PPO wrapper chain fused in, asked for with Agent.evaluate(persistent=True) (ppo_eval_config.mode = 2).

It runs k_act4's arithmetic, so on an act_kernel=4 context it must return the per-step path's bits and
leave the per-step path's env and wrapper state; against the CPU oracle it is held to twice the
per-step path's measured gap; where no persistent kernel covers the agent, mode = 2 is an error."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

MEAN, SAMPLE = ppo_amd.PPO_MEAN, ppo_amd.PPO_SAMPLE


def make(env, E, wrappers, kind=ppo_amd.PPO_NET_TANH_NORMAL, H=64):
    """(agent, env factory): env is an env id or (O, A) of the synthetic cheetah; the factory gives a fresh
    (SynthEnv, EnvWrappers | None). Every parameter is moved off its initial value (biases and log std
    start at zero, the head at gain 0.01)."""
    def envs():
        e = ppo_amd.SynthEnv(E, env_id=env) if isinstance(env, str) else ppo_amd.SynthEnv(E, *env)
        w = ppo_amd.EnvWrappers(E, e.O, 0.99) if wrappers else None
        if w is not None:
            e.attach_wrappers(w)
        return e, w
    e, w = envs()
    O, A = e.O, e.A
    e.close()
    hc = ppo_amd.HipConfig(kind, O, A, H, 64, 4, 1, 1, 0.99, 0.95, 0.2, 0.01, 0.5, 0.5, 1e-5, 1, 1, 1, 0, 1)
    ag = ppo_amd.Agent(hc, options="act_kernel=4" if kind == ppo_amd.PPO_NET_TANH_NORMAL else None)
    p = ppo_amd.init_params(ag.layout, seed=3)
    if kind == ppo_amd.PPO_NET_TANH_NORMAL:
        p = p + 0.05 * np.random.default_rng(4).standard_normal(p.size).astype(np.float32)
    ag.load_params(p)
    return ag, envs


# id: env, wrappers, E, nE, runs, sample type, step0, chunk_steps, least env steps
CASES = {
    "pendulum-ragged-mean": ("Pendulum-v1", True, 5, 3, 3, MEAN, 0, 0, 200),
    "pendulum-ragged-sample": ("Pendulum-v1", True, 5, 3, 3, SAMPLE, 12345, 0, 200),
    "cartpole-37-chunks": ("CartPoleContinuous-v1", True, 37, 37, 400, MEAN, 0, 48, 97),
    "cartpole-1029-rr16": ("CartPoleContinuous-v1", True, 1029, 1029, 2058, MEAN, 0, 48, 2),
    "quadrotor-sample": ("QuadrotorHover-v0", True, 5, 5, 5, SAMPLE, 12345, 0, 2),
    "cheetah-17-6-bare": ((17, 6), False, 2, 2, 2, MEAN, 0, 512, 1000),
    "cheetah-105-8": ((105, 8), True, 2, 2, 2, MEAN, 0, 512, 1000),
    "cheetah-376-17": ((376, 17), True, 2, 2, 2, MEAN, 0, 512, 1000),
    "acrobot": ("AcrobotContinuous-v1", True, 5, 5, 5, SAMPLE, 7, 0, 2),
    "reacher": ("ReacherPlanar-v0", True, 5, 5, 5, SAMPLE, 7, 0, 2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_persistent_bitwise_equals_per_step(case):
    env_spec, wrappers, E, nE, runs, mode, step0, chunk, least = CASES[case]
    ag, envs = make(env_spec, E, wrappers)
    out = []
    for how, info in ((dict(persistent=True), "eval=k_eval4"), (dict(per_step=True), "eval=per_step")):
        env, wr = envs()
        res = ag.evaluate(env, runs, mode, eval_seed=5, num_eval_envs=nE, step0=step0, chunk_steps=chunk, **how)
        assert ag.eval_info() == info
        # the state the call leaves: the wrapper chain's, and the env's through one further step of all E envs
        s = ppo_amd.lib().ppo_stream(ag.h)
        obs, rew, done = DeviceArray((E, env.O)), DeviceArray(E), DeviceArray(E)
        env.step(DeviceArray.from_numpy(np.full((E, env.A), 0.1, np.float32)), obs, rew, done, stream=s)
        st = wr.state() if wr is not None else {}
        out.append((res, {**{k: v.copy() for k, v in st.items()}, "obs": obs.numpy(), "rew": rew.numpy(), "done": done.numpy()}))
        env.close()
        if wr is not None:
            wr.close()
    ag.close()
    (fast, fs), (slow, ss) = out
    assert fast[0].size >= runs and fast[2] >= least and np.isfinite(fast[0]).all()
    np.testing.assert_array_equal(fast[0].view(np.uint32), slow[0].view(np.uint32))
    np.testing.assert_array_equal(fast[1], slow[1])
    assert fast[2] == slow[2]
    for k in ss:
        np.testing.assert_array_equal(fs[k].view(np.uint32), ss[k].view(np.uint32), err_msg=k)


# max |return(device) - return(oracle)| over the two episodes of the per-step path (mode = 1), measured
# on an MI355X: 6.676e-06 (oracle returns -4.53022051, -4.21090698). The bound is 2x that figure.
PER_STEP_ORACLE_GAP = 6.676e-06


def test_eval4_against_the_cpu_oracle():
    """E = 1, PPO_MEAN, two episodes, wrappers on, replayed on the CPU with orc_env_reset /
    orc_get_action_and_value (mode 2) / orc_env_step and the oracle's wrapper chain (orc_vwrap_*).
    The oracle steps the synthetic cheetah only (it has no Pendulum), so the env is the cheetah at
    O = 17, A = 6, as in test_gpu_eval.py's oracle test. The wrapper chain and the env are bit-exact
    with the oracle's, so the gap is the act gap carried through 2 001 steps.
    Measured gap of the per-step path (mode = 1, k_act4 + the env kernels that existed before k_eval4):
    6.676e-06 on returns of -4.53 and -4.21 (a dozen fp32 ulps: the normalised observations feed the
    act gap back through 2 001 steps); both paths are held to 2x that, and k_eval4 measured the same
    6.676e-06 (it is bitwise the per-step path)."""
    import oracle_lib as Orc
    O, A = 17, 6
    ag, envs = make((O, A), 1, True)
    L = Orc.layout_init(ppo_amd.PPO_NET_TANH_NORMAL, O, A, 64)
    p = ag.params()
    oenv = Orc.SynthEnv(1, O, A, wrappers=True)
    obs = oenv.reset(2)
    orets = []
    for k in range(2001):
        act, _, _, _ = Orc.get_action_and_value(L, p, obs, 2)
        obs, r, te, tr, ir, il = oenv.step(act)
        if tr[0] != 0:
            orets.append(ir[0])
    orets = np.array(orets, np.float64)
    assert orets.size == 2
    got = {}
    for how in ("per_step", "persistent"):
        env, wr = envs()
        got[how] = ag.evaluate(env, 2, MEAN, eval_seed=2, **{how: True})
        env.close()
        wr.close()
    ag.close()
    gs, gf = np.abs(got["per_step"][0] - orets).max(), np.abs(got["persistent"][0] - orets).max()
    print(f"oracle returns {orets}, per-step gap {gs:.3e}, persistent gap {gf:.3e}")
    assert gs <= 2 * PER_STEP_ORACLE_GAP and gf <= 2 * PER_STEP_ORACLE_GAP


def test_mode_2_refuses_what_no_persistent_kernel_covers():
    L = ppo_amd.lib()

    def call(ag, env, mode):
        cfg = ppo_amd.EvalConfig(MEAN, 2, 1, 2, 0, 0, mode)
        ret, ln = np.zeros(8, np.float32), np.zeros(8, np.int32)
        n, steps = C.c_int(), C.c_long()
        rc = L.ppo_evaluate_synth(ag.h, env.h, C.byref(cfg), ret.ctypes.data, ln.ctypes.data, 8, C.byref(n), C.byref(steps))
        return rc, L.ppo_last_error().decode()

    for spec, wrappers, words in (((17, 6), True, ("LayerNorm-Beta", "OP = 32", "A = 6", "wrapper chain")),
                                  ((105, 8), False, ("LayerNorm-Beta", "OP = 112", "A = 8"))):
        ag, envs = make(spec, 1, wrappers, kind=ppo_amd.PPO_NET_LN_BETA, H=256)
        env, wr = envs()
        rc, err = call(ag, env, 2)
        assert rc == -1 and "mode = 2" in err and all(w in err for w in words), err
        rc, err = call(ag, env, 3)
        assert rc == -1 and "bad chunk_steps / mode" in err
        with pytest.raises(ValueError, match="mutually exclusive"):
            ag.evaluate(env, 2, MEAN, persistent=True, per_step=True)
        env.close()
        if wr is not None:
            wr.close()
        ag.close()
    # where mode = 0 takes k_eval (AC agent, OP <= 32, no wrappers), mode = 2 takes it too: the same bits
    ag, envs = make((17, 6), 1, False, kind=ppo_amd.PPO_NET_LN_BETA, H=256)
    env, _ = envs()
    auto = ag.evaluate(env, 2, MEAN)
    assert ag.eval_info() == "eval=k_eval"
    asked = ag.evaluate(env, 2, MEAN, persistent=True)
    assert ag.eval_info() == "eval=k_eval"
    np.testing.assert_array_equal(auto[0].view(np.uint32), asked[0].view(np.uint32))
    assert list(auto[1]) == list(asked[1]) and auto[2] == asked[2]
    env.close()
    ag.close()
