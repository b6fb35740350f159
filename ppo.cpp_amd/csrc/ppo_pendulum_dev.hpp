// ppo_pendulum_dev.hpp — the device env kind PSYN_PENDULUM (Gymnasium's Pendulum-v1): the shared
// arithmetic of include/ppo_pendulum.h compiled for the device, and the reset draw from the env's
// Philox stream. Used by the per-step env kernels (ppo_kernels.hip) and, fused, by the persistent
// rollout / evaluation kernels (ppo_rollout.hip, ppo_eval.hip). Bit for bit the host env
// gymcpp/pendulum.h: no contraction, no device-library trigonometry.
#pragma once

#include "ppo_kernels.hpp"
#include "../../include/ppo_pendulum.h"

// reset number rc of the env keyed rs: counter (rc, i, 0, 0), i = 0 the angle, 1 the speed
// (the cheetah's reset draw of state element i)
PPO_DEV void pend_reset_dev(uint32_t rc, uint32_t rs, float* th, float* thd) {
  uint32_t r0[4], r1[4];
  philox4x32(rc, 0u, 0u, 0u, rs, 0x5EED5EEDu, r0);
  philox4x32(rc, 1u, 0u, 0u, rs, 0x5EED5EEDu, r1);
  pend_reset(u01(r0[0]), u01(r1[0]), th, thd);
}
