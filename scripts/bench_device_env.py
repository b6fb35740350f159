#!/usr/bin/env python3
"""AC agent on one of the device envs (Pendulum-v1, CartPoleContinuous-v1, ReacherPlanar-v0,
QuadrotorHover-v0, AcrobotContinuous-v1, or the synthetic cheetah as HalfCheetah-v5) at E = 4096, T = 128 (the metric
config's shape): the persistent rollout (k_rollout<NTO, 1, KIND>, or k_rollout_v for the cheetah at
E <= 512, + k_beta_logp + k_values) against the per-step path (rollout=per_step: k_act3 +
k_env_step<KIND> or k_synth_step per step), alternating, and the whole iteration (rollout + GAE +
update). Host clock around work that ends in a device synchronise; both trainers are warmed up first.
Medians only: no kernel trace is taken. Writes profiles/<name>/bench_<name>.txt and .json, <name>
being pendulum, cartpole, reacher, quadrotor, acrobot or cheetah.

  python scripts/bench_device_env.py --env_id ID [--num_envs 4096] [--num_steps 128] [--reps 10] [--out DIR]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppo.cpp_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import ppo_amd  # noqa: E402

SHORT = {"Pendulum-v1": "pendulum", "CartPoleContinuous-v1": "cartpole", "ReacherPlanar-v0": "reacher",
         "QuadrotorHover-v0": "quadrotor", "AcrobotContinuous-v1": "acrobot", "HalfCheetah-v5": "cheetah"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env_id", required=True, choices=sorted(SHORT))
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--num_steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = SHORT[a.env_id]
    out = a.out or os.path.join(ROOT, "profiles", name)
    E, T = a.num_envs, a.num_steps
    cfg = ppo_amd.ACPPOConfig(env_id=a.env_id, num_envs=E, num_steps=T, total_timesteps=E * T * (4 * a.reps + 8))
    trs = {"persistent": ppo_amd.Trainer(cfg), "per_step": ppo_amd.Trainer(cfg, options="rollout=per_step")}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"AC agent, {a.env_id} device env, E={E} T={T}: {E * T} env steps per rollout; {a.reps} alternating repetitions")
    for tr in trs.values():  # warm-up: code objects, first launches, the update's graph capture
        for _ in range(3):
            tr.iterate()
        tr.agent.sync()
    roll = {k: [] for k in trs}
    for _ in range(a.reps):
        for k, tr in trs.items():
            tr.agent.sync()
            t0 = time.perf_counter()
            tr.rollout()
            tr.agent.sync()
            roll[k].append(time.perf_counter() - t0)
            tr.agent.compute_gae(tr.next_obs, tr.next_done)  # keep both on the same trajectory of work
            tr.agent.update(tr.lr_now(), want_stats=False)
            tr.iteration += 1
    itr = []
    tr = trs["persistent"]
    for _ in range(a.reps):
        tr.agent.sync()
        t0 = time.perf_counter()
        tr.iterate()
        tr.agent.sync()
        itr.append(time.perf_counter() - t0)
    res = {"num_envs": E, "num_steps": T, "reps": a.reps}
    for k, v in roll.items():
        v = np.array(v)
        res[f"rollout_{k}_ms"] = {"median": float(np.median(v) * 1e3), "min": float(v.min() * 1e3), "max": float(v.max() * 1e3)}
        say(f"rollout {k:10s}: median {np.median(v) * 1e3:8.3f} ms (min {v.min() * 1e3:.3f}, max {v.max() * 1e3:.3f})  "
            f"{E * T / np.median(v) / 1e6:8.2f} M env steps/s  {np.median(v) / T * 1e6:7.2f} us per step")
    ratio = float(np.median(roll["per_step"]) / np.median(roll["persistent"]))
    v = np.array(itr)
    res["rollout_per_step_over_persistent"] = ratio
    res["iteration_ms"] = {"median": float(np.median(v) * 1e3), "min": float(v.min() * 1e3), "max": float(v.max() * 1e3)}
    res["iteration_env_steps_per_s"] = float(E * T / np.median(v))
    say(f"per_step / persistent rollout time: {ratio:.2f}x")
    say(f"whole iteration (rollout + GAE + update, 4 epochs x 4 minibatches): median {np.median(v) * 1e3:.3f} ms "
        f"(min {v.min() * 1e3:.3f}, max {v.max() * 1e3:.3f})  {E * T / np.median(v) / 1e6:.2f} M env steps/s")
    for t in trs.values():
        t.close()
    os.makedirs(out, exist_ok=True)
    open(os.path.join(out, f"bench_{name}.txt"), "w").write("\n".join(lines) + "\n")
    json.dump(res, open(os.path.join(out, f"bench_{name}.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
