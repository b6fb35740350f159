/*
 * ppo_pendulum.h — the arithmetic of Gymnasium's Pendulum-v1 (classic_control/pendulum.py), shared
 * by the host env (ppo.cpp_amd/gymcpp/pendulum.h), the device env kernels (ppo_kernels.hip,
 * ppo_rollout.hip, ppo_eval.hip) and the test driver (tests/native/pendulum_driver.cpp). Plain C.
 *
 * Host and device results are bit-identical: fp32 only, every fused multiply-add written as fmaf,
 * everything else with explicit parentheses and contraction off (host: -ffp-contract=off; device:
 * the pragma below), and sine / cosine from the polynomial pair of this file, never from libm or the
 * device library (those differ between host and device).
 *
 * One departure from Gymnasium: the stored angle is wrapped into [-pi, pi) after every step and at
 * reset. Gymnasium lets theta grow and normalises it inside the cost only; every use of theta (its
 * sine, its cosine, the normalised angle of the cost) is 2 pi-periodic, so the trajectory is the
 * same, and the wrapped angle keeps the polynomial's argument within |x| <= pi + 0.4.
 *
 * The helpers carry the prefix pend_ (tests/test_capi_cpu.py takes a ppo_ / psyn_ / pwrap_ call at
 * the start of a header line for an exported declaration).
 */
#ifndef PPO_PENDULUM_H
#define PPO_PENDULUM_H

#include <math.h>

#if defined(__HIPCC__)
#define PEND_FN static inline __host__ __device__
#else
#define PEND_FN static inline
#endif
#if defined(__clang__)
#define PEND_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PEND_NO_CONTRACT
#endif

#define PEND_OBS_DIM 3
#define PEND_ACT_DIM 1
#define PEND_MAX_STEPS 200
#define PEND_G 10.0f
#define PEND_M 1.0f
#define PEND_L 1.0f
#define PEND_DT 0.05f
#define PEND_MAX_SPEED 8.0f
#define PEND_MAX_TORQUE 2.0f
#define PEND_PI 3.14159274101257324f     /* float(pi) */
#define PEND_TWO_PI 6.28318548202514648f /* 2 * float(pi), exact */

/* sin(x) and cos(x) for |x| <= pi + 0.5. k = round(x * 2 / pi) in [-3, 3]; r = x - k pi / 2 by a
 * two-term Cody-Waite reduction (k * hi is exact inside the fmaf), |r| <= pi / 4 + 2^-22; then the
 * degree-7 / degree-8 minimax pair on that interval, swapped and negated by the quadrant k mod 4.
 * Only + - *, fmaf, floorf and conversions. */
PEND_FN void pend_sincos(float x, float* s_out, float* c_out) {
  PEND_NO_CONTRACT
  const float kf = floorf(fmaf(x, 0.636619746685028076f, 0.5f));
  float r = fmaf(-kf, 1.57079637050628662f, x);
  r = fmaf(-kf, -4.37113900018624283e-8f, r);
  const float z = (r * r);
  float ps = fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
  ps = fmaf(z, ps, -1.6666654611e-1f);
  const float sr = fmaf((r * z), ps, r);
  float pc = fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
  pc = fmaf(z, pc, 4.166664568298827e-2f);
  const float cr = fmaf((z * z), pc, fmaf(z, -0.5f, 1.0f));
  const int q = ((int)kf) & 3; /* two's complement: -1 & 3 = 3 */
  const float s = (q & 1) ? cr : sr;
  const float c = (q & 1) ? sr : cr;
  *s_out = (q & 2) ? (0.0f - s) : s;
  *c_out = ((q + 1) & 2) ? (0.0f - c) : c;
}

/* x in [-pi - 0.4, pi + 0.4] into [-pi, pi); both corrections are exact (Sterbenz) */
PEND_FN float pend_wrap(float x) {
  PEND_NO_CONTRACT
  return x >= PEND_PI ? (x - PEND_TWO_PI) : (x < (0.0f - PEND_PI) ? (x + PEND_TWO_PI) : x);
}

/* obs = (cos theta, sin theta, thetadot) */
PEND_FN void pend_obs(float th, float thd, float* obs) {
  float s, c;
  pend_sincos(th, &s, &c);
  obs[0] = c;
  obs[1] = s;
  obs[2] = thd;
}

/* reset: theta = pi (2 u0 - 1), thetadot = 2 u1 - 1, u0 / u1 uniform in (0, 1]
 * (u can round to 1: the wrap takes theta = +pi to -pi) */
PEND_FN void pend_reset(float u0, float u1, float* th, float* thd) {
  PEND_NO_CONTRACT
  *th = pend_wrap((PEND_PI * ((2.0f * u0) - 1.0f)));
  *thd = ((2.0f * u1) - 1.0f);
}

/* One step in place; returns the reward -cost. The torque is clipped to +-2 here, always (as
 * PendulumEnv.step's own np.clip), after whatever the vector env's clip_actions did. */
PEND_FN float pend_step(float* th_io, float* thd_io, float a, float* obs) {
  PEND_NO_CONTRACT
  const float th = *th_io, thd = *thd_io;
  const float u = fminf(fmaxf(a, (0.0f - PEND_MAX_TORQUE)), PEND_MAX_TORQUE);
  const float cost = (((th * th) + (0.1f * (thd * thd))) + (0.001f * (u * u)));
  float s, c;
  pend_sincos(th, &s, &c);
  /* 3 g / (2 l) = 15, 3 / (m l^2) = 3 */
  const float acc = fmaf(15.0f, s, (3.0f * u));
  const float nthd = fminf(fmaxf(fmaf(acc, PEND_DT, thd), (0.0f - PEND_MAX_SPEED)), PEND_MAX_SPEED);
  const float nth = pend_wrap(fmaf(nthd, PEND_DT, th));
  *th_io = nth;
  *thd_io = nthd;
  pend_obs(nth, nthd, obs);
  return (0.0f - cost);
}

#endif
