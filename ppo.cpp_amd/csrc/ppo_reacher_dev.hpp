// ppo_reacher_dev.hpp — the device env kind PSYN_REACHER (ReacherPlanar-v0: Reacher-v5's task
// definition over the textbook two-link arm; not MuJoCo's Reacher): the shared arithmetic of
// include/ppo_reacher.h compiled for the device, and the reset draw from the env's Philox stream.
// Used by the per-step env kernels (ppo_kernels.hip) and, fused, by the persistent rollout /
// evaluation kernels (ppo_rollout.hip, ppo_eval.hip). Bit for bit the host env gymcpp/reacher.h: no
// contraction, no device-library trigonometry, correctly rounded divisions and square roots.
#pragma once

#include "ppo_kernels.hpp"
#include "../../include/ppo_reacher.h"

// reset number rc of the env keyed rs: counter (rc, i, 0, 0), i = 0..5 for q1, q2, q1dot, q2dot and
// the goal's radius and angle (Pendulum's schedule, and the cheetah's reset draw of state element i)
PPO_DEV void reach_reset_dev(uint32_t rc, uint32_t rs, float* s6) {
  float u[REACH_STATE_DIM];
#pragma unroll
  for (int i = 0; i < REACH_STATE_DIM; ++i) {
    uint32_t r[4];
    philox4x32(rc, (uint32_t)i, 0u, 0u, rs, 0x5EED5EEDu, r);
    u[i] = u01(r[0]);
  }
  reach_reset(u, s6);
}
