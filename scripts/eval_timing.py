"""Writes bench_out/eval_timing.txt (the numbers of profiles/eval/eval_timing.txt).
Times the AC CLI's default evaluation (1 env, PPO_MEAN, 128 runs = 128 127 env steps, HalfCheetah shapes):
persistent (mode 0) against per-step (mode 1), alternating, three times each, and the host-driven loop once."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppo.cpp_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import ppo_amd
import test_gpu_eval as T
ag = T.make_agent()
env = ppo_amd.SynthEnv(1, 17, 6)
RUNS = 128
lines = []
def say(s):
    print(s, flush=True); lines.append(s)
# warm-up (module load, first launches)
ag.evaluate(env, 1); ag.evaluate(env, 1, per_step=True)
res = {}
for rep in range(3):
    for per_step in (False, True):
        ag.sync(); t0 = time.perf_counter()
        r = ag.evaluate(env, RUNS, ppo_amd.PPO_MEAN, eval_seed=2, per_step=per_step)
        dt = time.perf_counter() - t0
        res.setdefault(per_step, []).append(dt)
        say(f"rep {rep} {'per_step' if per_step else 'k_eval  '} {ag.eval_info()} steps={r[2]} n={r[0].size} time={dt*1e3:9.2f} ms  per env step={dt/r[2]*1e6:7.3f} us  avg_return={r[0].astype(np.float64).mean():.6f}")
        res[("r", per_step)] = r
assert np.array_equal(res[("r", False)][0].view(np.uint32), res[("r", True)][0].view(np.uint32))
for ch in (1024, 16384, 131072):
    ag.sync(); t0 = time.perf_counter()
    r = ag.evaluate(env, RUNS, ppo_amd.PPO_MEAN, eval_seed=2, chunk_steps=ch)
    dt = time.perf_counter() - t0
    say(f"k_eval chunk_steps={ch:6d} time={dt*1e3:9.2f} ms  per launched step={dt/(-(-r[2]//ch)*ch)*1e6:7.3f} us")
t0 = time.perf_counter()
h = T.host_loop(ag, ppo_amd.PPO_MEAN, 16)
dt = time.perf_counter() - t0
say(f"host loop (16 runs) steps={h[2]} time={dt*1e3:9.2f} ms  per env step={dt/h[2]*1e6:7.3f} us  -> 128 runs ~ {dt/h[2]*128128:.2f} s")
assert np.array_equal(h[0].view(np.uint32), res[("r", False)][0][:16].view(np.uint32))
say(f"median k_eval {np.median(res[False])*1e3:.2f} ms, per_step {np.median(res[True])*1e3:.2f} ms, ratio {np.median(res[True])/np.median(res[False]):.2f}x")
os.makedirs(os.path.join(ROOT, "bench_out"), exist_ok=True)
open(os.path.join(ROOT, "bench_out", "eval_timing.txt"), "w").write("\n".join(lines) + "\n")
