// ppo_quadrotor_dev.hpp — the device env kind PSYN_QUADROTOR (QuadrotorHover-v0: the textbook
// Newton-Euler quadrotor hovering at the origin; this project's own task, not a simulator's): the
// shared arithmetic of include/ppo_quadrotor.h compiled for the device, and the reset draw from the
// env's Philox stream. Used by the per-step env kernels (ppo_kernels.hip) and, fused, by the
// persistent rollout / evaluation kernels (ppo_rollout.hip, ppo_eval.hip). Bit for bit the host env
// gymcpp/quadrotor.h: no contraction, correctly rounded divisions and square roots.
#pragma once

#include "ppo_kernels.hpp"
#include "../../include/ppo_quadrotor.h"

// The tile shape (16-wide input tiles NTO, head tiles NHT) at which the fused kernels k_rollout,
// k_rollout4 and k_eval may be instantiated for an env kind: the cheetah at any shape, Pendulum-v1
// (O = 3, A = 1), CartPoleContinuous-v1 (O = 4, A = 1) and ReacherPlanar-v0 (O = 10, A = 2) in one
// input tile, QuadrotorHover-v0 (O = 18, A = 4) in two.
constexpr bool psyn_kind_tiles_ok(int kind, int nto, int nht) {
  return kind == PSYN_CHEETAH     ? true
         : kind == PSYN_QUADROTOR ? (nto == 2 && nht == 1)
                                  : (nto == 1 && nht == 1);
}
#define PSYN_KIND_TILES_MSG                                                                                      \
  "Pendulum-v1: O = 3, A = 1; CartPoleContinuous-v1: O = 4, A = 1; ReacherPlanar-v0: O = 10, A = 2 (one input " \
  "tile); QuadrotorHover-v0: O = 18, A = 4 (two input tiles)"

// reset number rc of the env keyed rs: counter (rc, i, 0, 0), i = 0..11 for p, v, the quaternion's
// vector part and omega (Pendulum's schedule, and the cheetah's reset draw of state element i).
// s13 may be an LDS row.
PPO_DEV void quad_reset_dev(uint32_t rc, uint32_t rs, float* s13) {
  float u[QUAD_RESET_DRAWS];
#pragma unroll
  for (int i = 0; i < QUAD_RESET_DRAWS; ++i) {
    uint32_t r[4];
    philox4x32(rc, (uint32_t)i, 0u, 0u, rs, 0x5EED5EEDu, r);
    u[i] = u01(r[0]);
  }
  quad_reset(u, s13);
}
