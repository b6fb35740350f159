/*
 * ppo_reacher.h — the arithmetic of ReacherPlanar-v0, a two-link planar arm with O = 10, A = 2.
 * This is not MuJoCo's Reacher. It takes Gymnasium Reacher-v5's task definition (observation layout,
 * reward, goal distribution, 50-step truncation, action space [-1, 1]^2) and puts the textbook
 * two-link manipulator equations under it: two uniform rods, joint torques G * a, joint damping, no
 * gravity (the arm moves in a horizontal plane), semi-implicit Euler in two substeps per env step.
 * Shared by the host env (ppo.cpp_amd/gymcpp/reacher.h), the device env kernels (ppo_kernels.hip,
 * ppo_rollout.hip, ppo_eval.hip) and the test driver (tests/native/reacher_driver.cpp). Plain C.
 *
 * Host and device results are bit-identical, by the rules of ppo_pendulum.h: fp32 only, every fused
 * multiply-add written as fmaf, everything else with explicit parentheses and contraction off, sine
 * and cosine from pend_sincos only. cos(q1 + q2) and sin(q1 + q2) come from the angle-addition
 * formulas on the two pend_sincos pairs, never from a sine of the sum (q1 + q2 leaves the polynomial's
 * domain). The divisions and the sqrtf are plain and correctly rounded on the host and on the device
 * (hipcc's default; no reciprocal or rsqrt approximation, no fast-math).
 *
 * The state is s = (q1, q2, q1dot, q2dot, gx, gy). The goal (gx, gy) is env state the dynamics never
 * touch: it is drawn at reset, uniform in the disc of radius 0.2, and survives every step. The
 * observation is (cos q1, cos q2, sin q1, sin q2, gx, gy, q1dot, q2dot, dx, dy) with d = tip - goal,
 * Reacher-v5's order. The reward is -|d| - 0.1 |a|^2 on the new state with the clipped action. The
 * episode never terminates; truncation after 50 steps is the caller's.
 *
 * One departure from the textbook integrator: the joint speeds are clipped to +-32 rad/s after each
 * substep, so that a substep moves an angle by at most 0.32 rad and the wrap into [-pi, pi) stays
 * inside pend_wrap's domain.
 *
 * Constants: derived in float64, rounded once to fp32 (float64 value, then the fp32 value used):
 *   l1 = 0.1                       0.10000000149011612
 *   l2 = 0.11                      0.10999999940395355
 *   a1 = 0.01736666666666667       0.017366666346788406   I1 + I2 + m1 r1^2 + m2 (l1^2 + r2^2)
 *   a2 = 0.0055000000000000005     0.0054999999701976776  m2 l1 r2
 *   2 a2 = 0.011000000000000001    0.010999999940395355
 *   a3 = 0.004033333333333333      0.0040333331562578678  I2 + m2 r2^2
 *   G = 0.2                        0.20000000298023224    torque gain
 *   D = 0.02                       0.019999999552965164   joint damping
 *   dt = 0.01                      0.0099999997764825821  substep
 * with m1 = m2 = 1, r_i = l_i / 2, I_i = m_i l_i^2 / 12 (uniform rods).
 * det M = a1 a3 - a3^2 - a2^2 cos^2 q2 >= 2.3528e-5 > 0 at every q2.
 *
 * The helpers carry the prefix reach_ (tests/test_capi_cpu.py takes a ppo_ / psyn_ / pwrap_ call at
 * the start of a header line for an exported declaration).
 */
#ifndef PPO_REACHER_H
#define PPO_REACHER_H

#include "ppo_pendulum.h"

#define REACH_OBS_DIM 10
#define REACH_ACT_DIM 2
#define REACH_STATE_DIM 6
#define REACH_MAX_STEPS 50
#define REACH_SUBSTEPS 2
#define REACH_L1 0.1f
#define REACH_L2 0.11f
#define REACH_A1 0.01736666666666667f
#define REACH_A2 0.0055f
#define REACH_2A2 0.011f
#define REACH_A3 0.004033333333333333f
#define REACH_GAIN 0.2f
#define REACH_DAMP 0.02f
#define REACH_DT 0.01f
#define REACH_MAX_SPEED 32.0f
#define REACH_CTRL_W 0.1f
#define REACH_GOAL_R 0.2f

/* obs = (cos q1, cos q2, sin q1, sin q2, gx, gy, q1dot, q2dot, dx, dy); returns |d| */
PEND_FN float reach_obs(const float* s, float* obs) {
  PEND_NO_CONTRACT
  float s1, c1, s2, c2;
  pend_sincos(s[0], &s1, &c1);
  pend_sincos(s[1], &s2, &c2);
  const float c12 = fmaf(c1, c2, (0.0f - (s1 * s2)));
  const float s12 = fmaf(s1, c2, (c1 * s2));
  const float dx = (fmaf(REACH_L2, c12, (REACH_L1 * c1)) - s[4]);
  const float dy = (fmaf(REACH_L2, s12, (REACH_L1 * s1)) - s[5]);
  obs[0] = c1;
  obs[1] = c2;
  obs[2] = s1;
  obs[3] = s2;
  obs[4] = s[4];
  obs[5] = s[5];
  obs[6] = s[2];
  obs[7] = s[3];
  obs[8] = dx;
  obs[9] = dy;
  return sqrtf(fmaf(dx, dx, (dy * dy)));
}

/* reset from six uniforms in (0, 1]: q = 0.2 u - 0.1, qdot = 0.01 u - 0.005,
 * goal = rho (cos phi, sin phi) with rho = 0.2 sqrt(u4), phi = wrap(pi (2 u5 - 1)): uniform in the
 * disc, no rejection loop */
PEND_FN void reach_reset(const float* u, float* s) {
  PEND_NO_CONTRACT
  s[0] = fmaf(0.2f, u[0], -0.1f);
  s[1] = fmaf(0.2f, u[1], -0.1f);
  s[2] = fmaf(0.01f, u[2], -0.005f);
  s[3] = fmaf(0.01f, u[3], -0.005f);
  const float rho = (REACH_GOAL_R * sqrtf(u[4]));
  const float phi = pend_wrap((PEND_PI * ((2.0f * u[5]) - 1.0f)));
  float sp, cp;
  pend_sincos(phi, &sp, &cp);
  s[4] = (rho * cp);
  s[5] = (rho * sp);
}

/* one semi-implicit Euler substep of the two-link arm under the torques G * (u0, u1) */
PEND_FN void reach_substep(float* s, float u0, float u1) {
  PEND_NO_CONTRACT
  const float q1 = s[0], q2 = s[1], v1 = s[2], v2 = s[3];
  float s2, c2;
  pend_sincos(q2, &s2, &c2);
  const float m11 = fmaf(REACH_2A2, c2, REACH_A1);
  const float m12 = fmaf(REACH_A2, c2, REACH_A3);
  const float m22 = REACH_A3;
  const float h = (REACH_A2 * s2);
  const float t1 = fmaf(h, fmaf((2.0f * v1), v2, (v2 * v2)), fmaf((0.0f - REACH_DAMP), v1, (REACH_GAIN * u0)));
  const float t2 = fmaf((0.0f - h), (v1 * v1), fmaf((0.0f - REACH_DAMP), v2, (REACH_GAIN * u1)));
  const float det = fmaf(m11, m22, (0.0f - (m12 * m12)));
  const float acc1 = (fmaf(m22, t1, (0.0f - (m12 * t2))) / det);
  const float acc2 = (fmaf(m11, t2, (0.0f - (m12 * t1))) / det);
  const float nv1 = fminf(fmaxf(fmaf(REACH_DT, acc1, v1), (0.0f - REACH_MAX_SPEED)), REACH_MAX_SPEED);
  const float nv2 = fminf(fmaxf(fmaf(REACH_DT, acc2, v2), (0.0f - REACH_MAX_SPEED)), REACH_MAX_SPEED);
  s[0] = pend_wrap(fmaf(REACH_DT, nv1, q1));
  s[1] = pend_wrap(fmaf(REACH_DT, nv2, q2));
  s[2] = nv1;
  s[3] = nv2;
}

/* One env step in place on s = (q1, q2, q1dot, q2dot, gx, gy); writes the observation of the new
 * state and returns the reward. Both actions are clipped to [-1, 1] here, always, after whatever the
 * vector env's clip_actions did (a NaN action gives -1, as fminf / fmaxf give it). The goal slots
 * are read, never written. */
PEND_FN float reach_step(float* s, const float* a, float* obs) {
  PEND_NO_CONTRACT
  const float u0 = fminf(fmaxf(a[0], -1.0f), 1.0f);
  const float u1 = fminf(fmaxf(a[1], -1.0f), 1.0f);
  for (int k = 0; k < REACH_SUBSTEPS; ++k) reach_substep(s, u0, u1);
  const float dist = reach_obs(s, obs);
  return ((0.0f - dist) - (REACH_CTRL_W * fmaf(u0, u0, (u1 * u1))));
}

#endif
