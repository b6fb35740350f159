"""Writes profiles/rollout_wide/rollout_wide_timing.txt ("k_rollout_w"), or into the directory
given as the first argument. Times ppo_rollout_synth of the AC agent at Humanoid width (LayerNorm-Beta,
H = 256, O = 376, A = 17, T = 128) on an update=off context at E = 16, 256 and 4 096: the persistent path
(k_rollout_w + k_beta_logp + the critic launch) against set_rollout_mode(per_step=True), in one process,
alternating, three times each after a warm-up of both. One repetition is CALLS consecutive rollouts and
the stream synchronisation after the last (a single rollout is a few milliseconds). Before the timing the
two paths run once each from the same reset and their storage is compared bit for bit."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppo.cpp_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import ppo_amd
from ppo_amd import DeviceArray
O, A, T, CALLS = 376, 17, 128, 64
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rollout_wide")
lines = []
def say(s):
    print(s, flush=True); lines.append(s)
for E in (16, 256, 4096):
    hc = ppo_amd.HipConfig(ppo_amd.PPO_NET_LN_BETA, O, A, 256, E, T, 1, 1, 0.99, 0.95, 0.2, 0.01, 0.5, 0.5, 1e-5, 1, 1, 1, 0, 1)
    ag = ppo_amd.Agent(hc, options="update=off")  # the AC agent exists at A = 17 as an acting-only context
    ag.load_params(ppo_amd.init_params(ag.layout, seed=3, env_id="Humanoid-v4"))
    env = ppo_amd.SynthEnv(E, O, A)
    nobs, ndone, act, rew = DeviceArray((E, O)), DeviceArray(E), DeviceArray((E, A)), DeviceArray(E)
    def run(per_step, calls):
        ag.set_rollout_mode(per_step)
        for _ in range(calls):
            ppo_amd.check(ppo_amd.lib().ppo_rollout_synth(ag.h, env.h, nobs.ptr, ndone.ptr, act.ptr, rew.ptr))
        ag.sync()
    snaps = []
    for per_step in (False, True):  # warm-up of both, and the comparison at this size
        env.reset(5, nobs, ndone, ppo_amd.lib().ppo_stream(ag.h))
        run(per_step, 1)
        snaps.append([ag.buffer(getattr(ppo_amd, b), (T, E, A) if b == "BUF_ACTIONS" else (T, E)).numpy().view(np.uint32)
                      for b in ("BUF_ACTIONS", "BUF_LOGPROBS", "BUF_VALUES", "BUF_REWARDS", "BUF_DONES")] + [nobs.numpy().view(np.uint32)])
    assert all(np.array_equal(x, y) for x, y in zip(*snaps)), "the two paths differ"
    res = {}
    for rep in range(3):
        for per_step in (False, True):
            ag.sync(); t0 = time.perf_counter()
            run(per_step, CALLS)
            dt = time.perf_counter() - t0
            res.setdefault(per_step, []).append(dt)
            say(f"O={O} A={A} T={T} E={E} rep {rep} {ag.rollout_info():20s} calls={CALLS} time={dt*1e3:9.2f} ms  per rollout={dt/CALLS*1e3:8.3f} ms  per env step={dt/CALLS/T*1e6:7.3f} us")
    mp, ms = np.median(res[False]), np.median(res[True])
    say(f"E={E}: median k_rollout_w {mp/CALLS*1e3:.3f} ms per rollout ({mp/CALLS/T*1e6:.3f} us/step), per_step {ms/CALLS*1e3:.3f} ms ({ms/CALLS/T*1e6:.3f} us/step), "
        f"ratio {ms/mp:.2f}x; every persistent repetition faster than every per-step one: {max(res[False]) < min(res[True])}")
    ag.close(); env.close()
os.makedirs(out_dir, exist_ok=True)
open(os.path.join(out_dir, "rollout_wide_timing.txt"), "w").write("\n".join(lines) + "\n")
