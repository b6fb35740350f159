"""k_rollout_w (csrc/ppo_rollout_wide.hip): the AC agent's persistent rollout kernel at Humanoid width
(LayerNorm-Beta, H = 256, OP = 384, 17 <= A <= 24, the cheetah-shaped env without a wrapper chain).

It runs k_act3<LN_BETA, 24, 3>'s chain and k_synth_step_wide's step and stores what the per-step path
stores, so after every rollout the storage, next_obs / next_done, the env state and the episode totals
must be the per-step path's bits; ppo_rollout_info names the path; against the CPU oracle the stored
log-probs and values are held to twice the per-step path's measured gap. The contexts are acting-only
(update=off: the default refuses A >= 13 at hidden 256), so the test sets the iteration itself."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

SEED = 11
BUFS = {"obs": "BUF_OBS", "actions": "BUF_ACTIONS", "logprobs": "BUF_LOGPROBS", "values": "BUF_VALUES",
        "rewards": "BUF_REWARDS", "dones": "BUF_DONES"}
# id: O, A, E, T
CASES = {
    "one-env-across-the-autoreset": (376, 17, 1, 400),  # 3 x 400 steps: the reset at step 1 000, next_done carried
    "ragged-o373": (373, 17, 5, 8),                     # O % 4 != 0, 5 of 16 rows
    "full-op-a20": (384, 20, 17, 8),                    # O = OP, 640 Beta items, a second workgroup of one env
    "three-workgroups": (376, 17, 33, 3),               # the t * E strides
}


class Side:
    """One acting-only context with its own env and next_obs / next_done."""

    def __init__(self, O, A, E, T, options, wrappers=False):
        hc = ppo_amd.HipConfig(ppo_amd.PPO_NET_LN_BETA, O, A, 256, E, T, 1, 1, 0.99, 0.95, 0.2, 0.01, 0.5, 0.5, 1e-5, 1, 1, 1, 0, 1)
        self.ag, self.shape = ppo_amd.Agent(hc, options=options), (O, A, E, T)
        rng = np.random.default_rng(4)  # every parameter off its initial value, an obs mean / std that is not the identity
        L = self.ag.layout
        p0 = ppo_amd.init_params(L, seed=3, obs_mean=0.1 * rng.standard_normal(O), obs_std=rng.uniform(0.5, 2.0, O))
        p = p0 + 0.05 * rng.standard_normal(p0.size).astype(np.float32)
        for off, n in ((L.hi, 1), (L.lo, 1), (L.omean, O), (L.ostd, O)):
            p[off:off + n] = p0[off:off + n]
        self.ag.load_params(p)
        self.env = ppo_amd.SynthEnv(E, O, A)
        self.wr = ppo_amd.EnvWrappers(E, O, 0.99) if wrappers else None
        if wrappers:
            self.env.attach_wrappers(self.wr)
        self.next_obs, self.next_done = DeviceArray((E, O)), DeviceArray(E)
        self.scratch = DeviceArray((E, A)), DeviceArray(E)
        self.env.reset(SEED, self.next_obs, self.next_done, ppo_amd.lib().ppo_stream(self.ag.h))

    def rollout(self, it):
        """Rollout number it; returns everything it leaves. The env state is read through one further step
        of all envs into scratch outputs (the next rollout then starts from an env one step ahead of
        next_obs, on both sides alike)."""
        O, A, E, T = self.shape
        self.ag.set_iteration(it)
        ppo_amd.check(ppo_amd.lib().ppo_rollout_synth(self.ag.h, self.env.h, self.next_obs.ptr, self.next_done.ptr,
                                                      self.scratch[0].ptr, self.scratch[1].ptr))
        self.ag.sync()
        out = {k: self.ag.buffer(getattr(ppo_amd, b), (T, E, O) if k == "obs" else (T, E, A) if k == "actions" else (T, E)).numpy()
               for k, b in BUFS.items()}
        out["next_obs"], out["next_done"] = self.next_obs.numpy(), self.next_done.numpy()
        obs, rew, done = DeviceArray((E, O)), DeviceArray(E), DeviceArray(E)
        self.env.step(DeviceArray.from_numpy(np.full((E, A), 0.1, np.float32)), obs, rew, done, stream=ppo_amd.lib().ppo_stream(self.ag.h))
        self.ag.sync()
        out.update(env_obs=obs.numpy(), env_rew=rew.numpy(), env_done=done.numpy(), totals=np.array(self.env.episode_stats(), np.float32))
        return out, self.ag.rollout_info()

    def close(self):
        self.ag.close()
        self.env.close()
        if self.wr:
            self.wr.close()


@functools.lru_cache(maxsize=None)
def rollouts(case):
    """Three consecutive rollouts of the case on an auto and a per-step context: [(auto, per-step)] and the
    parameters; computed once, never modified."""
    sides = [Side(*CASES[case], "update=off"), Side(*CASES[case], "update=off,rollout=per_step")]
    assert sides[0].ag.rollout_info() == "rollout=none"
    res = [tuple(s.rollout(it) for s in sides) for it in range(3)]
    params = sides[0].ag.params()
    for s in sides:
        s.close()
    return res, params


@pytest.mark.parametrize("case", list(CASES))
def test_persistent_rollout_bitwise_equals_per_step(case):
    O, A, E, T = CASES[case]
    res, _ = rollouts(case)
    finished = 0.0
    for it, ((fast, finfo), (slow, sinfo)) in enumerate(res):
        assert finfo == "rollout=k_rollout_w" and sinfo == "rollout=per_step"
        for k in slow:
            np.testing.assert_array_equal(fast[k].view(np.uint32), slow[k].view(np.uint32), err_msg=f"rollout {it}: {k}")
        assert np.isfinite(fast["logprobs"]).all() and np.isfinite(fast["values"]).all()
        finished += fast["totals"][2]
    if 3 * T >= 1000:  # the truncation at step 1 000 and the reset after it happened inside a rollout
        assert finished == E and sum(f["dones"].sum() for (f, _), _ in res) == E


def test_what_does_not_take_the_kernel():
    side = Side(376, 17, 2, 2, "update=off", wrappers=True)
    assert side.rollout(0)[1] == "rollout=per_step"
    side.close()
    tr = ppo_amd.Trainer(ppo_amd.ACPPOConfig(env_id="HalfCheetah-v5", num_envs=16, num_steps=4, num_minibatches=1,
                                             update_epochs=1, total_timesteps=64))
    tr.rollout()
    assert tr.agent.rollout_info() == "rollout=k_rollout"
    tr.close()


# max |stored - oracle| over the first 64 rows of the first case's first rollout, per-step path, measured on an
# MI355X: log-probs 8.345e-06 (oracle log-probs in [-3.63, 4.43]), values 8.941e-07 (oracle values in
# [-0.077, 1.029]). The bounds are 2x these figures.
PER_STEP_ORACLE_GAP = {"logprobs": 8.345e-06, "values": 8.941e-07}


def test_rollout_wide_against_the_cpu_oracle():
    """The stored obs and actions of the first 64 steps (O = 376, A = 17, E = 1), through
    orc_get_action_and_value with the action given: both paths' stored log-probs and values are held to
    2x the per-step path's measured gap (log-probs 8.345e-06, values 8.941e-07); k_rollout_w measured the
    same 8.345e-06 and 8.941e-07 (it is bitwise the per-step path)."""
    import oracle_lib as Orc
    O, A, E, T = CASES["one-env-across-the-autoreset"]
    res, params = rollouts("one-env-across-the-autoreset")
    (fast, _), (slow, _) = res[0]
    obs, act = slow["obs"][:64, 0], slow["actions"][:64, 0]
    _, olp, _, ov = Orc.get_action_and_value(Orc.layout_init(1, O, A, 256), params, obs, 1, act)
    gaps = {}
    for k, ref in (("logprobs", olp), ("values", ov)):
        gaps[k] = [np.abs(side[k][:64, 0] - ref.astype(np.float64)).max() for side in (slow, fast)]
        print(f"{k}: oracle range [{ref.min():.6f}, {ref.max():.6f}], per-step gap {gaps[k][0]:.3e}, persistent gap {gaps[k][1]:.3e}")
    for k, g in gaps.items():
        assert max(g) <= 2 * PER_STEP_ORACLE_GAP[k], k
