#!/usr/bin/env python3
"""CPU reference for "the trainer learns QuadrotorHover-v0" (tests/test_gpu_quadrotor.py::test_it_learns
and test_it_learns_ac): the first real task wider than one 16-wide input tile (O = 18, A = 4), a
rigid-body quadrotor that hovers at the origin; it terminates (|p|^2 > 9) and truncates (500 steps).

The loop of scripts/pendulum_learning_ref.py (its run_seed(), evaluate(), argument parser and main()
are used as they are) over the host env gymcpp::QuadrotorHover behind SeqVectorEnv +
RecordEpisodeStatistics (tests/native/quadrotor_driver.cpp built as a shared object,
tests/quadrotor_common.py HostQuad): oracle_lib.get_action_and_value / gae / update at O = 18, A = 4,
and for the PPO agent the oracle's wrapper chain (oracle_lib.VecWrappers) over the 18-wide
observation, which gets the env's termination flag: NormalizeReward restarts its return accumulator
after a termination.

Per seed it measures the mean-action return over the first 64 evaluation episodes (all envs reset
with eval_seed) before and after training and writes tests/golden/quadrotor/learning_ref[_ac].json.
The config must satisfy, on this reference alone: in every seed
trained - untrained >= 2 * (max - min of the untrained returns across seeds).

  python scripts/quadrotor_learning_ref.py [--agent ppo|ac] [--num_envs 64] ... [--out PATH] [--curve] [--jobs 3]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "ppo.cpp_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pendulum_learning_ref as P  # noqa: E402
import quadrotor_common as qc  # noqa: E402

ENV, OD, AD = qc.ENV_ID, qc.OD, qc.AD
EVAL_EPISODES = P.EVAL_EPISODES
DEFAULTS = dict(num_envs=64, num_steps=128, total_timesteps=64 * 128 * 20, num_minibatches=32, update_epochs=10,
                learning_rate=3e-3, gamma=0.99, gae_lambda=0.95)
HostQuad = qc.HostQuad


def parser():
    ap = P.parser()
    ap.set_defaults(out=None, **DEFAULTS)
    return ap


def main():
    a = parser().parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "tests", "golden", "quadrotor", "learning_ref.json" if a.agent == "ppo" else "learning_ref_ac.json")
    P.main(a, ENV, (OD, AD), HostQuad)


if __name__ == "__main__":
    main()
