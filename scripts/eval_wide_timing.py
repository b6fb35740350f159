"""Writes profiles/eval_wide/eval_wide_timing.txt ("k_eval_w"), or into the directory given
as the first argument. Times the AC agent's evaluation at Humanoid width (LayerNorm-Beta, H = 256, O = 376,
A = 17; PPO_MEAN, 128 runs), persistent (mode 2, k_eval_w) against per-step (mode 1), in one process,
alternating, three times each after a warm-up of both:
  a. one env (ac:965-1001): 128 127 env steps;
  b. nE = E = 16 (one full workgroup): 8 008 env steps of 16 envs.
Each timed call ends in the call's own stream synchronisation (the event read-out)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppo.cpp_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import ppo_amd
O, A, RUNS = 376, 17, 128
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "eval_wide")
lines = []
def say(s):
    print(s, flush=True); lines.append(s)
hc = ppo_amd.HipConfig(ppo_amd.PPO_NET_LN_BETA, O, A, 256, 64, 4, 1, 1, 0.99, 0.95, 0.2, 0.01, 0.5, 0.5, 1e-5, 1, 1, 1, 0, 1)
ag = ppo_amd.Agent(hc, options="update=off")  # the AC agent exists at A = 17 as an acting-only context
ag.load_params(ppo_amd.init_params(ag.layout, seed=3, env_id="Humanoid-v4"))
for E in (1, 16):
    env = ppo_amd.SynthEnv(E, O, A)
    for how in ("persistent", "per_step"):  # warm-up (module load, first launches)
        ag.evaluate(env, E, ppo_amd.PPO_MEAN, num_eval_envs=E, **{how: True})
    res, last = {}, {}
    for rep in range(3):
        for how in ("persistent", "per_step"):
            ag.sync(); t0 = time.perf_counter()
            r = ag.evaluate(env, RUNS, ppo_amd.PPO_MEAN, eval_seed=2, num_eval_envs=E, **{how: True})
            dt = time.perf_counter() - t0
            res.setdefault(how, []).append(dt)
            last[how] = r
            say(f"O={O} A={A} nE={E} rep {rep} {how:10s} {ag.eval_info()} steps={r[2]} n={r[0].size} time={dt*1e3:9.2f} ms  per step={dt/r[2]*1e6:7.3f} us  avg_return={r[0].astype(np.float64).mean():.6f}")
    env.close()
    assert np.array_equal(last["persistent"][0].view(np.uint32), last["per_step"][0].view(np.uint32))
    mp, ms, n = np.median(res["persistent"]), np.median(res["per_step"]), last["per_step"][2]
    say(f"nE={E}: median k_eval_w {mp*1e3:.2f} ms ({mp/n*1e6:.3f} us/step), per_step {ms*1e3:.2f} ms ({ms/n*1e6:.3f} us/step), ratio {ms/mp:.2f}x")
ag.close()
os.makedirs(out_dir, exist_ok=True)
open(os.path.join(out_dir, "eval_wide_timing.txt"), "w").write("\n".join(lines) + "\n")
