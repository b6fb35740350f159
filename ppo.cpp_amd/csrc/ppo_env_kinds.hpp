// ppo_env_kinds.hpp — the device env kinds with dynamics of their own, each defined once:
//   PSYN_PENDULUM   Pendulum-v1            Gymnasium's pendulum.py
//   PSYN_CARTPOLE   CartPoleContinuous-v1  Gymnasium's cartpole.py with a continuous force; it terminates
//   PSYN_REACHER    ReacherPlanar-v0       Reacher-v5's task over the textbook two-link arm (not MuJoCo's)
//   PSYN_QUADROTOR  QuadrotorHover-v0      this project's hover task over the textbook Newton-Euler
//                                          quadrotor; it terminates
//   PSYN_ACROBOT    AcrobotContinuous-v1   Gymnasium's acrobot.py ("book", RK4) with a continuous torque;
//                                          it terminates, on success
// DevEnv<KIND> is a kind's shape, its reset from the env's Philox stream and its step: the shared
// arithmetic of include/ppo_{pendulum,cartpole,reacher,quadrotor,acrobot}.h compiled for the device, bit for
// bit the host envs gymcpp/{pendulum,cartpole,reacher,quadrotor,acrobot}.h (no contraction, no device-library
// trigonometry, correctly rounded divisions and square roots). kEnvKinds is the same kinds for the
// host, one row each, and dispatch_env_kind turns a run-time kind into the compile-time one.
// Used by the per-step env kernels k_env_reset / k_env_step (ppo_kernels.hip), by env_lane_step
// (ppo_rollout_common.hpp) inside the persistent kernels k_rollout, k_rollout4 (ppo_rollout.hip) and
// k_eval (ppo_eval.hip), and by the C API (ppo_capi.hip).
// PSYN_CHEETAH has no DevEnv: it exists at any (O, A) and its step is spread over an env's lanes
// (k_synth_step / k_synth_step_wide, chee_lanes_step of ppo_rollout_common.hpp, k_rollout4's element
// loop). Its arithmetic is include/ppo_cheetah.h, shared with the host env
// gymcpp/synthetic_cheetah.h; the device forms of its pieces (chee_reset_elem, chee_clip,
// chee_reward_clip) are below, next to the reset stream every kind draws from.
#pragma once

#include "ppo_kernels.hpp"
#include "../../include/ppo_cheetah.h"
#include "../../include/ppo_pendulum.h"
#include "../../include/ppo_cartpole.h"
#include "../../include/ppo_reacher.h"
#include "../../include/ppo_quadrotor.h"
#include "../../include/ppo_acrobot.h"

#include <type_traits>

// the uniforms of reset number rc of the env keyed rs: counter (rc, i, 0, 0) for draw i, every kind's
// reset stream. All kinds share one second key word; the cheetah's header names it (CHEE_RESET_KEY)
// because the cheetah is the kind whose host env takes it from a shared header, and the host envs of
// the other kinds (gymcpp/{pendulum,cartpole,reacher,quadrotor,acrobot}.h) spell the same value themselves.
constexpr uint32_t kEnvResetKey = CHEE_RESET_KEY;
PPO_DEV float env_reset_draw(uint32_t rc, uint32_t rs, int i) {
  uint32_t r[4];
  philox4x32(rc, (uint32_t)i, 0u, 0u, rs, kEnvResetKey, r);
  return u01(r[0]);
}
template <int N>
PPO_DEV void env_reset_draws(uint32_t rc, uint32_t rs, float (&u)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) u[i] = env_reset_draw(rc, rs, i);
}

// The synthetic cheetah on the device (include/ppo_cheetah.h): state element i of reset number rc,
// and the reward of a step from the env's unclipped actions ar[0..A-1] (clip_actions applied here, per
// dimension, as for the element update)
PPO_DEV float chee_reset_elem(uint32_t rc, uint32_t rs, int i) { return chee_reset_value(env_reset_draw(rc, rs, i)); }
PPO_DEV float chee_clip(float a, float lo, float hi) { return fminf(fmaxf(a, lo), hi); }
PPO_DEV float chee_reward_clip(float q0_new, float q0_old, const float* ar, int A, float lo, float hi) {
  float ctrl = 0.0f;
  for (int k = 0; k < A; ++k) ctrl = chee_ctrl_add(ctrl, chee_clip(ar[k], lo, hi));
  return chee_reward_ctrl(q0_new, q0_old, ctrl);
}

// DevEnv<KIND>:
//   O, A        observation and action widths
//   S           state floats kept in the env's row of q ([E][O]; the slots S..O-1 stay zero)
//   MAX_STEPS   truncation; TERMINATES: whether step can raise its termination flag
//   NTO, NHT    the tile shape (16-wide input tiles, head tiles) the persistent kernels are built at
//   IN_PLACE    the persistent kernels step the env directly on its LDS rows (s = its row of Q, obs =
//               its row of XO) instead of register copies
//   reset(rc, rs, s, obs)           the state and observation of reset number rc of the env keyed rs
//   step(s, act, obs, term) -> reward   one step in place on s from the A actions (after clip_actions;
//                                   the dynamics clip to their own range themselves); term = 1.0f | 0.0f
template <int KIND>
struct DevEnv;

template <>
struct DevEnv<PSYN_PENDULUM> {  // s = (theta, thetadot); draws: the angle, the speed
  static constexpr int O = PEND_OBS_DIM, A = PEND_ACT_DIM, S = 2, MAX_STEPS = PEND_MAX_STEPS, NTO = 1, NHT = 1;
  static constexpr bool TERMINATES = false, IN_PLACE = false;
  PPO_DEV static void reset(uint32_t rc, uint32_t rs, float* s, float* obs) {
    float u[2];
    env_reset_draws(rc, rs, u);
    pend_reset(u[0], u[1], &s[0], &s[1]);
    pend_obs(s[0], s[1], obs);
  }
  PPO_DEV static float step(float* s, const float* act, float* obs, float* term) {
    *term = 0.0f;
    return pend_step(&s[0], &s[1], act[0], obs);
  }
};

template <>
struct DevEnv<PSYN_CARTPOLE> {  // s = (x, xdot, theta, thetadot), which is the observation, raw
  static constexpr int O = CART_OBS_DIM, A = CART_ACT_DIM, S = CART_OBS_DIM, MAX_STEPS = CART_MAX_STEPS, NTO = 1, NHT = 1;
  static constexpr bool TERMINATES = true, IN_PLACE = false;
  PPO_DEV static void reset(uint32_t rc, uint32_t rs, float* s, float* obs) {
    float u[CART_OBS_DIM];
    env_reset_draws(rc, rs, u);
    cart_reset(u, s);
#pragma unroll
    for (int i = 0; i < CART_OBS_DIM; ++i) obs[i] = s[i];
  }
  PPO_DEV static float step(float* s, const float* act, float* obs, float* term) {
    const float rw = cart_step(s, act[0], term);
#pragma unroll
    for (int i = 0; i < CART_OBS_DIM; ++i) obs[i] = s[i];
    return rw;
  }
};

template <>
struct DevEnv<PSYN_REACHER> {  // s = (q1, q2, q1dot, q2dot, gx, gy); draws: those four, the goal's radius and angle
  static constexpr int O = REACH_OBS_DIM, A = REACH_ACT_DIM, S = REACH_STATE_DIM, MAX_STEPS = REACH_MAX_STEPS, NTO = 1, NHT = 1;
  static constexpr bool TERMINATES = false, IN_PLACE = false;
  PPO_DEV static void reset(uint32_t rc, uint32_t rs, float* s, float* obs) {
    float u[REACH_STATE_DIM];
    env_reset_draws(rc, rs, u);
    reach_reset(u, s);  // a new goal with the new episode
    reach_obs(s, obs);
  }
  // The goal slots s[4], s[5] are set by a reset only: reach_step reads them (reach_obs) and writes
  // s[0..3] (reach_substep), so a caller that stores all S floats back stores the goal it loaded.
  PPO_DEV static float step(float* s, const float* act, float* obs, float* term) {
    *term = 0.0f;
    return reach_step(s, act, obs);
  }
};

template <>
struct DevEnv<PSYN_QUADROTOR> {  // s = (p, v, quaternion, omega); draws: p, v, the quaternion's vector part, omega
  static constexpr int O = QUAD_OBS_DIM, A = QUAD_ACT_DIM, S = QUAD_STATE_DIM, MAX_STEPS = QUAD_MAX_STEPS, NTO = 2, NHT = 1;
  // in place: 13 + 18 values in registers next to the persistent kernels' resident weights would spill
  static constexpr bool TERMINATES = true, IN_PLACE = true;
  PPO_DEV static void reset(uint32_t rc, uint32_t rs, float* s, float* obs) {
    float u[QUAD_RESET_DRAWS];
    env_reset_draws(rc, rs, u);
    quad_reset(u, s);
    quad_obs(s, obs);
  }
  PPO_DEV static float step(float* s, const float* act, float* obs, float* term) { return quad_step(s, act, obs, term); }
};

template <>
struct DevEnv<PSYN_ACROBOT> {  // s = (theta1, theta2, theta1dot, theta2dot); draws: those four
  static constexpr int O = ACRO_OBS_DIM, A = ACRO_ACT_DIM, S = ACRO_STATE_DIM, MAX_STEPS = ACRO_MAX_STEPS, NTO = 1, NHT = 1;
  static constexpr bool TERMINATES = true, IN_PLACE = false;
  PPO_DEV static void reset(uint32_t rc, uint32_t rs, float* s, float* obs) {
    float u[ACRO_STATE_DIM];
    env_reset_draws(rc, rs, u);
    acro_reset(u, s);
    (void)acro_obs(s, obs);
  }
  PPO_DEV static float step(float* s, const float* act, float* obs, float* term) { return acro_step(s, act[0], obs, term); }
};

// the tile shape at which k_rollout, k_rollout4 and k_eval may be instantiated for an env kind: the
// cheetah at any shape, every other kind at its own
template <int KIND, int NTO, int NHT>
constexpr bool psyn_kind_tiles_ok() {
  if constexpr (KIND == PSYN_CHEETAH) return true;
  else return NTO == DevEnv<KIND>::NTO && NHT == DevEnv<KIND>::NHT;
}
#define PSYN_KIND_TILES_MSG "an env kind with a DevEnv is built at its DevEnv<KIND>::NTO input tiles and NHT head tiles only"

// The same kinds for the host: one row per kind, taken from its DevEnv.
struct EnvKindRow {
  const char* env_id;
  const char* kind_name;
  int kind, O, A;
  float act_lo, act_hi;  // the env's action space (clip_actions)
  int max_steps;
  bool terminates;
  bool zero_q;           // O > S: q has unused slots, defined (zero) from creation on; the persistent kernels carry them along
};
template <int KIND>
constexpr EnvKindRow env_kind_row(const char* env_id, const char* kind_name, float act_lo, float act_hi) {
  using D = DevEnv<KIND>;
  return {env_id, kind_name, KIND, D::O, D::A, act_lo, act_hi, D::MAX_STEPS, D::TERMINATES, D::O > D::S};
}
constexpr EnvKindRow kEnvKinds[] = {
    env_kind_row<PSYN_PENDULUM>("Pendulum-v1", "PSYN_PENDULUM", -PEND_MAX_TORQUE, PEND_MAX_TORQUE),
    env_kind_row<PSYN_CARTPOLE>("CartPoleContinuous-v1", "PSYN_CARTPOLE", -1.0f, 1.0f),
    env_kind_row<PSYN_REACHER>("ReacherPlanar-v0", "PSYN_REACHER", -1.0f, 1.0f),
    env_kind_row<PSYN_QUADROTOR>("QuadrotorHover-v0", "PSYN_QUADROTOR", -1.0f, 1.0f),
    env_kind_row<PSYN_ACROBOT>("AcrobotContinuous-v1", "PSYN_ACROBOT", -1.0f, 1.0f),
};
// the row of a kind; null for PSYN_CHEETAH and for a number that is no kind
inline const EnvKindRow* env_kind_row_of(int kind) {
  for (const EnvKindRow& r : kEnvKinds)
    if (r.kind == kind) return &r;
  return nullptr;
}

// f(std::integral_constant<int, KIND>{}) for the kind's DevEnv; -1 for PSYN_CHEETAH and for a number
// that is no kind (f returns 0 or a negative launch code of its own)
template <typename F>
static int dispatch_env_kind(int kind, F&& f) {
  switch (kind) {
    case PSYN_PENDULUM: return f(std::integral_constant<int, PSYN_PENDULUM>{});
    case PSYN_CARTPOLE: return f(std::integral_constant<int, PSYN_CARTPOLE>{});
    case PSYN_REACHER: return f(std::integral_constant<int, PSYN_REACHER>{});
    case PSYN_QUADROTOR: return f(std::integral_constant<int, PSYN_QUADROTOR>{});
    case PSYN_ACROBOT: return f(std::integral_constant<int, PSYN_ACROBOT>{});
  }
  return -1;
}
