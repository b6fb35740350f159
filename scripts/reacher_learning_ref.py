#!/usr/bin/env python3
"""CPU reference for "the trainer learns ReacherPlanar-v0" (tests/test_gpu_reacher.py::test_it_learns):
the first real task with a two-dimensional action (a two-link planar arm with Reacher-v5's task
definition over the textbook two-link equations; not MuJoCo's Reacher).

The loop of scripts/pendulum_learning_ref.py (its run_seed(), evaluate(), argument parser and main()
are used as they are) over the host env gymcpp::ReacherPlanar behind SeqVectorEnv + RecordEpisodeStatistics
(tests/native/reacher_driver.cpp built as a shared object): oracle_lib.get_action_and_value / gae /
update at A = 2, and for the PPO agent the oracle's wrapper chain (oracle_lib.VecWrappers) over the
ten-wide observation. The env never terminates.

Per seed it measures the mean-action return over 64 evaluation episodes (all envs reset with
eval_seed: one 50-step chunk, every env finishes on the same step) before and after training and
writes tests/golden/reacher/learning_ref[_ac].json. The config must satisfy, on this reference
alone: in every seed  trained - untrained >= 2 * (max - min of the untrained returns across seeds).

  python scripts/reacher_learning_ref.py [--agent ppo|ac] [--num_envs 64] ... [--out PATH] [--curve]
  python scripts/reacher_learning_ref.py --agent ac --total_timesteps 491520 --jobs 3   # the AC fixture: 60 iterations
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "ppo.cpp_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pendulum_learning_ref as P  # noqa: E402

ENV, OD, AD = "ReacherPlanar-v0", 10, 2
EVAL_EPISODES = P.EVAL_EPISODES
DEFAULTS = dict(num_envs=64, num_steps=128, total_timesteps=64 * 128 * 20, num_minibatches=32, update_epochs=10,
                learning_rate=3e-3, gamma=0.99, gae_lambda=0.95)


class HostReacher:
    """SeqVectorEnv over RecordEpisodeStatistics(gymcpp::ReacherPlanar), clip_actions on."""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            d = tempfile.mkdtemp(prefix="reachdrv")
            so = os.path.join(d, "libreachdrv.so")
            subprocess.run(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-shared", "-fPIC", "-pthread",
                            os.path.join(ROOT, "tests", "native", "reacher_driver.cpp"), "-o", so], check=True)
            cls._lib = C.CDLL(so)
            cls._lib.reachdrv_create.restype = C.c_void_p
            cls._lib.reachdrv_create.argtypes = [C.c_int, C.c_int]
            cls._lib.reachdrv_destroy.argtypes = [C.c_void_p]
            cls._lib.reachdrv_reset.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            cls._lib.reachdrv_step.argtypes = [C.c_void_p] + [C.c_void_p] * 6
        return cls._lib

    def __init__(self, E):
        self.E = E
        self.h = self.lib().reachdrv_create(E, 1)
        self.obs = np.zeros((E, OD), np.float32)
        self.rew, self.done, self.ret, self.len = (np.zeros(E, np.float32) for _ in range(4))

    def reset(self, seed):
        self.lib().reachdrv_reset(self.h, seed, self.obs.ctypes.data)
        return self.obs.copy()

    def step(self, act):
        act = np.ascontiguousarray(act, np.float32)
        assert act.shape == (self.E, AD)
        self.lib().reachdrv_step(self.h, act.ctypes.data, self.obs.ctypes.data, self.rew.ctypes.data, self.done.ctypes.data,
                                 self.ret.ctypes.data, self.len.ctypes.data)
        return self.obs.copy(), self.rew.copy(), self.done.copy(), self.ret.copy(), self.len.copy()

    def close(self):
        if self.h:
            self.lib().reachdrv_destroy(self.h)
            self.h = None


def parser():
    ap = P.parser()
    ap.set_defaults(out=None, **DEFAULTS)
    return ap


def main():
    a = parser().parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "tests", "golden", "reacher", "learning_ref.json" if a.agent == "ppo" else "learning_ref_ac.json")
    P.main(a, ENV, (OD, AD), HostReacher)


if __name__ == "__main__":
    main()
