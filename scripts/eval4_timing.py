"""Writes bench_out/eval4_timing.txt (the numbers of profiles/eval4/eval4_timing.txt).
Times the PPO agent's evaluation, persistent (mode 2, k_eval4) against per-step (mode 1), in one process,
alternating, three times each after a warm-up of both:
  a. cheetah O = 17, A = 6, H = 64, wrappers on, 1 env, 128 runs of PPO_MEAN (128 127 env steps);
  b. CartPoleContinuous-v1, nE = E = 64, wrappers on, chunk_steps = 1 (the learning test's protocol:
     one host synchronisation per env step on both paths), 2 000 runs.
Each timed call ends in the call's own stream synchronisation (the event read-out)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppo.cpp_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import ppo_amd
lines = []
def make(spec, E):
    """(tanh-Normal agent on an act_kernel=4 context, factory of a fresh env with fresh wrappers)"""
    def envs():
        e = ppo_amd.SynthEnv(E, env_id=spec) if isinstance(spec, str) else ppo_amd.SynthEnv(E, *spec)
        w = ppo_amd.EnvWrappers(E, e.O, 0.99)
        e.attach_wrappers(w)
        return e, w
    e, w = envs()
    hc = ppo_amd.HipConfig(ppo_amd.PPO_NET_TANH_NORMAL, e.O, e.A, 64, 64, 4, 1, 1, 0.99, 0.95, 0.2, 0.01, 0.5, 0.5, 1e-5, 1, 1, 1, 0, 1)
    e.close(); w.close()
    ag = ppo_amd.Agent(hc, options="act_kernel=4")
    p = ppo_amd.init_params(ag.layout, seed=3)
    ag.load_params(p + 0.05 * np.random.default_rng(4).standard_normal(p.size).astype(np.float32))
    return ag, envs
def say(s):
    print(s, flush=True); lines.append(s)
for name, spec, E, runs, chunk in (("cheetah17x6 E=1", (17, 6), 1, 128, 0), ("cartpole E=64 chunk=1", "CartPoleContinuous-v1", 64, 2000, 1)):
    ag, envs = make(spec, E)
    env, wr = envs()
    for how in ("persistent", "per_step"):  # warm-up (module load, first launches)
        ag.evaluate(env, 1, ppo_amd.PPO_MEAN, num_eval_envs=E, chunk_steps=chunk, **{how: True})
    env.close(); wr.close()
    res, last = {}, {}
    for rep in range(3):
        for how in ("persistent", "per_step"):
            env, wr = envs()  # fresh normaliser statistics: every call computes the same episodes
            ag.sync(); t0 = time.perf_counter()
            r = ag.evaluate(env, runs, ppo_amd.PPO_MEAN, eval_seed=2, num_eval_envs=E, chunk_steps=chunk, **{how: True})
            dt = time.perf_counter() - t0
            env.close(); wr.close()
            res.setdefault(how, []).append(dt)
            last[how] = r
            say(f"{name} rep {rep} {how:10s} {ag.eval_info()} steps={r[2]} n={r[0].size} time={dt*1e3:9.2f} ms  per step={dt/r[2]*1e6:7.3f} us  avg_return={r[0].astype(np.float64).mean():.6f}")
    assert np.array_equal(last["persistent"][0].view(np.uint32), last["per_step"][0].view(np.uint32))
    mp, ms = np.median(res["persistent"]), np.median(res["per_step"])
    say(f"{name}: median k_eval4 {mp*1e3:.2f} ms, per_step {ms*1e3:.2f} ms, ratio {ms/mp:.2f}x")
    ag.close()
os.makedirs(os.path.join(ROOT, "bench_out"), exist_ok=True)
open(os.path.join(ROOT, "bench_out", "eval4_timing.txt"), "w").write("\n".join(lines) + "\n")
