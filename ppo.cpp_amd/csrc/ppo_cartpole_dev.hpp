// ppo_cartpole_dev.hpp — the device env kind PSYN_CARTPOLE (CartPoleContinuous-v1): the shared
// arithmetic of include/ppo_cartpole.h compiled for the device, and the reset draw from the env's
// Philox stream. Used by the per-step env kernels (ppo_kernels.hip) and, fused, by the persistent
// rollout / evaluation kernels (ppo_rollout.hip, ppo_eval.hip). Bit for bit the host env
// gymcpp/cartpole.h: no contraction, no device-library trigonometry, correctly rounded divisions.
#pragma once

#include "ppo_kernels.hpp"
#include "../../include/ppo_cartpole.h"

// reset number rc of the env keyed rs: counter (rc, i, 0, 0), i = 0..3 for x, xdot, theta, thetadot
// (Pendulum's schedule, and the cheetah's reset draw of state element i)
PPO_DEV void cart_reset_dev(uint32_t rc, uint32_t rs, float* s4) {
  float u[CART_OBS_DIM];
#pragma unroll
  for (int i = 0; i < CART_OBS_DIM; ++i) {
    uint32_t r[4];
    philox4x32(rc, (uint32_t)i, 0u, 0u, rs, 0x5EED5EEDu, r);
    u[i] = u01(r[0]);
  }
  cart_reset(u, s4);
}
