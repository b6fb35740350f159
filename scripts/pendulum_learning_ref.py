#!/usr/bin/env python3
"""CPU reference for "the trainer learns Pendulum-v1" (tests/test_gpu_pendulum.py::test_it_learns).

Runs the trainer loop on the CPU from pieces that exist independently of the GPU code:
  * the host env gymcpp::Pendulum behind SeqVectorEnv + RecordEpisodeStatistics, through
    tests/native/pendulum_driver.cpp built as a shared object;
  * oracle_lib.get_action_and_value (SAMPLE with the project's Philox keys (seed, rank, env, step),
    MEAN for the bootstrap value and the evaluation), oracle_lib.gae, oracle_lib.update (Feistel
    permutations, clip_grad_norm_, Adam);
  * for the PPO agent the oracle's wrapper chain (oracle_lib.VecWrappers: NormalizeObservation ->
    clamp -> NormalizeReward -> clamp), which is what ppo_amd.Trainer attaches for that agent.
Initial parameters are ppo_amd.init_params(seed), the learning rate anneals linearly, as Trainer does.

Per seed it measures the mean-action return over 64 evaluation episodes (envs reset with eval_seed)
before and after training and writes tests/golden/pendulum/learning_ref.json. The config must satisfy,
on this reference alone: in every seed  trained - untrained >= 2 * (max - min of the untrained returns
across seeds).

  python scripts/pendulum_learning_ref.py [--agent ppo] [--num_envs 64] ... [--out PATH] [--curve]
"""
import argparse
import ctypes as C
import datetime
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "ppo.cpp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle_lib as O  # noqa: E402

ENV, OD, AD = "Pendulum-v1", 3, 1
EVAL_EPISODES = 64


class HostPendulum:
    """SeqVectorEnv over RecordEpisodeStatistics(gymcpp::Pendulum), clip_actions on."""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            d = tempfile.mkdtemp(prefix="pendrv")
            so = os.path.join(d, "libpendrv.so")
            subprocess.run(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-shared", "-fPIC", "-pthread",
                            os.path.join(ROOT, "tests", "native", "pendulum_driver.cpp"), "-o", so], check=True)
            cls._lib = C.CDLL(so)
            cls._lib.pendrv_create.restype = C.c_void_p
            cls._lib.pendrv_create.argtypes = [C.c_int, C.c_int]
            cls._lib.pendrv_destroy.argtypes = [C.c_void_p]
            cls._lib.pendrv_reset.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            cls._lib.pendrv_step.argtypes = [C.c_void_p] + [C.c_void_p] * 6
        return cls._lib

    def __init__(self, E):
        self.E = E
        self.h = self.lib().pendrv_create(E, 1)
        self.obs = np.zeros((E, OD), np.float32)
        self.rew, self.done, self.ret, self.len = (np.zeros(E, np.float32) for _ in range(4))

    def reset(self, seed):
        self.lib().pendrv_reset(self.h, seed, self.obs.ctypes.data)
        return self.obs.copy()

    def step(self, act):
        act = np.ascontiguousarray(act, np.float32)
        self.lib().pendrv_step(self.h, act.ctypes.data, self.obs.ctypes.data, self.rew.ctypes.data, self.done.ctypes.data,
                               self.ret.ctypes.data, self.len.ctypes.data)
        return self.obs.copy(), self.rew.copy(), self.done.copy(), self.ret.copy(), self.len.copy()

    def close(self):
        if self.h:
            self.lib().pendrv_destroy(self.h)
            self.h = None


class WrappedEnv:
    """The env the trainer sees: the host env (HostPendulum, or another class with its interface whose
    step() may also return the termination flags, after the rewards), under the PPO wrapper chain for
    the PPO agent."""

    def __init__(self, E, wrapped, gamma, host=HostPendulum, od=OD):
        self.env = host(E)
        self.wrap = O.VecWrappers(E, od, gamma) if wrapped else None
        self.was_done = np.zeros(E, np.float32)

    def reset(self, seed):
        obs = self.env.reset(seed)
        self.was_done[:] = 0
        return self.wrap.reset(obs) if self.wrap else obs

    def step(self, act):
        out = self.env.step(act)
        obs, rew, done, ret, ln = out if len(out) == 5 else out[:2] + out[3:]
        term = np.zeros_like(rew) if len(out) == 5 else out[2]  # Pendulum never terminates
        if self.wrap:  # the step after a done is the autoreset: its reward (0) bypasses NormalizeReward
            obs, rew = self.wrap.step(obs, rew, term, self.was_done)
        self.was_done = done
        return obs, rew, done, ret, ln

    def close(self):
        self.env.close()


def evaluate(env, L, p, eval_seed):
    """Mean-action episodes of all envs after reset(eval_seed), until EVAL_EPISODES have finished
    (every episode of that step is kept: ppo_evaluate_synth's rule)."""
    obs = env.reset(eval_seed)
    rets = []
    while len(rets) < EVAL_EPISODES:
        a, _, _, _ = O.get_action_and_value(L, p, obs, 2)
        obs, _, _, ret, ln = env.step(a)
        rets += [float(r) for r, n in zip(ret, ln) if n > 0]
    return float(np.mean(rets)), len(rets)


def run_seed(a, seed, curve=False, max_iters=None, want_params=False, env_id=ENV, dims=(OD, AD), host=HostPendulum):
    """max_iters / want_params: stop early and return the parameters (to compare one iteration with the GPU).
    env_id / dims / host: the task (scripts/cartpole_learning_ref.py runs this loop over its own host env)."""
    ENV, (OD, AD) = env_id, dims
    import ppo_amd
    kind = ppo_amd.PPO_NET_TANH_NORMAL if a.agent == "ppo" else ppo_amd.PPO_NET_LN_BETA
    H = 64 if a.agent == "ppo" else 256
    E, T = a.num_envs, a.num_steps
    L = O.layout_init(kind, OD, AD, H)
    p = ppo_amd.init_params(ppo_amd.agent_layout(kind, OD, AD, H), seed=seed, env_id=ENV)
    env = WrappedEnv(E, a.agent == "ppo", a.gamma, host, OD)
    env.reset(seed)  # Trainer's constructor resets the env once (the observation normaliser sees it)
    untrained, n_eval = evaluate(env, L, p, a.eval_seed)
    obs = env.reset(seed)
    done = np.zeros(E, np.float32)
    m, v, step = np.zeros(L.P, np.float32), np.zeros(L.P, np.float32), 0
    lcfg = O.LossCfg(a.clip_coef, a.ent_coef, a.vf_coef, 1, 1)
    iters = a.total_timesteps // (E * T)
    pts = []
    for it in range(iters if max_iters is None else min(iters, max_iters)):
        frac = np.float32(1.0) - np.float32(it) / np.float32(iters)
        lr = float(np.float32(frac * np.float32(a.learning_rate)))
        bo = np.zeros((T, E, OD), np.float32); ba = np.zeros((T, E, AD), np.float32)
        bl, br, bd, bv = (np.zeros((T, E), np.float32) for _ in range(4))
        fin = []
        for t in range(T):
            bo[t], bd[t] = obs, done
            act, lp, _, val = O.get_action_and_value(L, p, obs, 0, seed=seed, rank=0, env_base=0, step_id=it * T + t)
            ba[t], bl[t], bv[t] = act, lp, val
            obs, br[t], done, ret, ln = env.step(act)
            fin += [float(r) for r, n in zip(ret, ln) if n > 0]
        _, _, _, nv = O.get_action_and_value(L, p, obs, 2)
        adv, rets = O.gae(br, bv, bd, nv, done, a.gamma, a.gae_lambda)
        p, m, v, step, _ = O.update(L, p, m, v, step, bo.reshape(-1, OD), ba.reshape(-1, AD), bl.reshape(-1), adv.reshape(-1),
                                    rets.reshape(-1), bv.reshape(-1), a.update_epochs, a.num_minibatches, lr, a.max_grad_norm,
                                    a.adam_eps, lcfg, seed=seed, rank=0, epoch_counter0=it * a.update_epochs)
        if fin:
            pts.append([(it + 1) * E * T, float(np.mean(fin))])
            if curve:
                print(f"  seed {seed} step {(it + 1) * E * T}: mean training return {np.mean(fin):.1f}", flush=True)
    if want_params:
        env.close()
        return p
    trained, _ = evaluate(env, L, p, a.eval_seed)
    env.close()
    return {"seed": seed, "untrained": untrained, "trained": trained, "eval_episodes": n_eval, "training_returns": pts}


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agent", choices=["ppo", "ac"], default="ppo")
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--eval_seed", type=int, default=1000)
    ap.add_argument("--num_envs", type=int, default=64)
    ap.add_argument("--num_steps", type=int, default=200)
    ap.add_argument("--total_timesteps", type=int, default=64 * 200 * 20)
    ap.add_argument("--num_minibatches", type=int, default=32)
    ap.add_argument("--update_epochs", type=int, default=10)
    ap.add_argument("--learning_rate", type=float, default=3e-3)
    ap.add_argument("--gamma", type=float, default=0.9)
    ap.add_argument("--gae_lambda", type=float, default=0.95)
    ap.add_argument("--clip_coef", type=float, default=0.2)
    ap.add_argument("--ent_coef", type=float, default=0.0)
    ap.add_argument("--vf_coef", type=float, default=0.5)
    ap.add_argument("--max_grad_norm", type=float, default=0.5)
    ap.add_argument("--adam_eps", type=float, default=1e-5)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pendulum", "learning_ref.json"))
    ap.add_argument("--curve", action="store_true")
    ap.add_argument("--jobs", type=int, default=1, help="seeds run in this many processes (the results do not change)")
    return ap


def main(a=None, env_id=ENV, dims=(OD, AD), host=HostPendulum, min_improvement=None):
    """min_improvement: the improvement every seed must also reach, for a task whose untrained returns
    are all equal (spread 0: scripts/acrobot_learning_ref.py); written to the file as required_improvement."""
    a = a or parser().parse_args()
    t0 = time.time()
    if getattr(a, "jobs", 1) > 1:  # one forked process per seed, before any library is loaded
        import multiprocessing as mp
        with mp.get_context("fork").Pool(min(a.jobs, len(a.seeds))) as pool:
            runs = pool.starmap(run_seed, [(a, s, a.curve, None, False, env_id, dims, host) for s in a.seeds])
    else:
        runs = [run_seed(a, s, a.curve, env_id=env_id, dims=dims, host=host) for s in a.seeds]
    un = [r["untrained"] for r in runs]
    spread = max(un) - min(un)
    imp = [r["trained"] - r["untrained"] for r in runs]
    ok = all(d >= 2 * spread and (min_improvement is None or d >= min_improvement) for d in imp)
    cfg = {k: getattr(a, k) for k in ("agent", "eval_seed", "num_envs", "num_steps", "total_timesteps", "num_minibatches",
                                      "update_epochs", "learning_rate", "gamma", "gae_lambda", "clip_coef", "ent_coef",
                                      "vf_coef", "max_grad_norm", "adam_eps")}
    out = {"env_id": env_id, "config": cfg, "seeds": a.seeds, "runs": runs, "untrained_spread": spread,
           "min_improvement": min(imp), "condition_met": ok, "eval_episodes": EVAL_EPISODES,
           "date": datetime.date.today().isoformat()}
    if min_improvement is not None:
        out["required_improvement"] = min_improvement
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for r in runs:
        print(f"seed {r['seed']}: untrained {r['untrained']:.1f} -> trained {r['trained']:.1f}")
    print(f"untrained spread {spread:.1f}, min improvement {min(imp):.1f}, condition met: {ok}; {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
