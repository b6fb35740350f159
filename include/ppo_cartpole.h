/*
 * ppo_cartpole.h — the arithmetic of CartPoleContinuous-v1: Gymnasium's CartPole-v1
 * (classic_control/cartpole.py: Barto-Sutton-Anderson dynamics, kinematics_integrator = "euler",
 * sutton_barto_reward = False) with one change, the force is force_mag * clip(a, -1, 1) from one
 * continuous action instead of +-force_mag from a discrete one. Shared by the host env
 * (ppo.cpp_amd/gymcpp/cartpole.h), the device env kernels (ppo_kernels.hip, ppo_rollout.hip,
 * ppo_eval.hip) and the test driver (tests/native/cartpole_driver.cpp). Plain C.
 *
 * Host and device results are bit-identical, by the rules of ppo_pendulum.h: fp32 only, every fused
 * multiply-add written as fmaf, everything else with explicit parentheses and contraction off, sine
 * and cosine from pend_sincos (|theta| stays far inside its domain: an env whose |theta| passes
 * 12 degrees terminates and is reset before its next step). The two divisions are plain fp32
 * divisions, correctly rounded on the host and on the device (hipcc's default; no reciprocal
 * approximation, no fast-math). The constant factors of cartpole.py that are not divisions of a
 * variable (polemass_length / total_mass, length * masspole / total_mass, 4 / 3 * length) are folded
 * into fp32 constants.
 *
 * The state is (x, xdot, theta, thetadot) and is the observation, raw. The episode terminates when
 * |x| > 2.4 or |theta| > 12 * 2 pi / 360, tested on the new state in fp32; the reward is 1 on every
 * step, the terminating one included; truncation after 500 steps is the caller's.
 *
 * The helpers carry the prefix cart_ (tests/test_capi_cpu.py takes a ppo_ / psyn_ / pwrap_ call at
 * the start of a header line for an exported declaration).
 */
#ifndef PPO_CARTPOLE_H
#define PPO_CARTPOLE_H

#include "ppo_pendulum.h"

#define CART_OBS_DIM 4
#define CART_ACT_DIM 1
#define CART_MAX_STEPS 500
#define CART_GRAVITY 9.8f
#define CART_TOTAL_MASS 1.1f          /* masscart 1.0 + masspole 0.1 */
#define CART_POLEMASS_LENGTH 0.05f    /* masspole 0.1 * half-length 0.5 */
#define CART_FORCE_MAG 10.0f
#define CART_TAU 0.02f
#define CART_X_THRESHOLD 2.4f
#define CART_THETA_THRESHOLD 0.20943951023931953f /* 12 * 2 pi / 360 */
/* length * 4 / 3 and length * masspole / total_mass (the denominator of thetaacc),
 * polemass_length / total_mass (the pole's share of xacc) */
#define CART_DEN0 0.66666666666666663f
#define CART_DEN1 0.045454545454545456f
#define CART_PML_OVER_M 0.045454545454545456f

/* reset: every state value is 0.1 u - 0.05, u uniform in (0, 1] (so each lies in (-0.05f, 0.05f]:
 * 0.1f is exactly 2 * 0.05f) */
PEND_FN void cart_reset(const float* u, float* s) {
  PEND_NO_CONTRACT
  for (int i = 0; i < CART_OBS_DIM; ++i) s[i] = fmaf(0.1f, u[i], -0.05f);
}

/* One step in place on s = (x, xdot, theta, thetadot); returns the reward (1.0f, always) and writes
 * the termination flag (1.0f | 0.0f). The action is clipped to [-1, 1] here, always, after whatever
 * the vector env's clip_actions did (a NaN action gives force -10, as fminf / fmaxf give it). */
PEND_FN float cart_step(float* s, float a, float* term) {
  PEND_NO_CONTRACT
  const float x = s[0], xd = s[1], th = s[2], thd = s[3];
  const float force = (CART_FORCE_MAG * fminf(fmaxf(a, -1.0f), 1.0f));
  float sn, cs;
  pend_sincos(th, &sn, &cs);
  const float temp = (fmaf((CART_POLEMASS_LENGTH * (thd * thd)), sn, force) / CART_TOTAL_MASS);
  const float num = fmaf(CART_GRAVITY, sn, (0.0f - (cs * temp)));
  const float den = fmaf((0.0f - CART_DEN1), (cs * cs), CART_DEN0);
  const float thacc = (num / den);
  const float xacc = fmaf((0.0f - (CART_PML_OVER_M * thacc)), cs, temp);
  /* euler: the positions move by the old velocities */
  const float nx = fmaf(CART_TAU, xd, x);
  const float nxd = fmaf(CART_TAU, xacc, xd);
  const float nth = fmaf(CART_TAU, thd, th);
  const float nthd = fmaf(CART_TAU, thacc, thd);
  s[0] = nx;
  s[1] = nxd;
  s[2] = nth;
  s[3] = nthd;
  const int out = (nx < (0.0f - CART_X_THRESHOLD)) || (nx > CART_X_THRESHOLD) ||
                  (nth < (0.0f - CART_THETA_THRESHOLD)) || (nth > CART_THETA_THRESHOLD);
  *term = out ? 1.0f : 0.0f;
  return 1.0f;
}

#endif
