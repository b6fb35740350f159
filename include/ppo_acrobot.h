/*
 * ppo_acrobot.h — the arithmetic of AcrobotContinuous-v1: Gymnasium's Acrobot-v1
 * (classic_control/acrobot.py, book_or_nips = "book", torque_noise_max = 0) with one change, the
 * torque is clip(a, -1, 1) from one continuous action instead of one of {-1, 0, 1}. Shared by the
 * host env (ppo.cpp_amd/gymcpp/acrobot.h), the device env kernels (ppo_kernels.hip, ppo_rollout.hip,
 * ppo_eval.hip) and the test driver (tests/native/acrobot_driver.cpp). Plain C.
 *
 * Host and device results are bit-identical, by the rules of ppo_pendulum.h: fp32 only, every fused
 * multiply-add written as fmaf, everything else with explicit parentheses and contraction off, sine
 * and cosine from pend_sincos, and the three divisions of a derivative evaluation plain fp32
 * divisions, correctly rounded on the host and on the device (hipcc's default; no reciprocal
 * approximation, no fast-math).
 *
 * The state is s = (theta1, theta2, theta1dot, theta2dot). One env step is one classical RK4 step of
 * ACRO_DT with the torque held: four evaluations of acro_deriv, the speeds not clipped between the
 * stages. Then both angles are wrapped into [-pi, pi) and both speeds clipped to +-4 pi / +-9 pi.
 * Between the stages the angles leave pend_sincos's domain (|x| <= pi + 0.5) by several radians, so
 * every angle goes through acro_reduce first. sin and cos of theta1 + theta2 come from the
 * angle-addition formulas, never from pend_sincos of the sum. Gymnasium's cos(x - pi / 2) is sin x.
 *
 * The episode terminates when the tip is above the bar, -cos theta1' - cos(theta1' + theta2') > 1 on
 * the new state in fp32; the reward is -1 on every step but the terminating one, which pays 0;
 * truncation after 500 steps is the caller's. The observation is
 * (cos theta1, sin theta1, cos theta2, sin theta2, theta1dot, theta2dot).
 *
 * With m1 = m2 = 1, l1 = 1, lc1 = lc2 = 0.5, I1 = I2 = 1, g = 9.8 the constant factors of
 * acrobot.py's _dsdt are folded in float64 and rounded to fp32 once (ACRO_* below, each with its
 * float64 value and the fp32 number it becomes):
 *   d1   = m1 lc1^2 + m2 (l1^2 + lc2^2 + 2 l1 lc2 cos theta2) + I1 + I2 = 3.5 + cos theta2
 *   d2   = m2 (lc2^2 + l1 lc2 cos theta2) + I2                         = 1.25 + 0.5 cos theta2
 *   phi2 = m2 lc2 g sin(theta1 + theta2)                               = 4.9 sin(theta1 + theta2)
 *   phi1 = -m2 l1 lc2 theta2dot^2 sin theta2 - 2 m2 l1 lc2 theta2dot theta1dot sin theta2
 *          + (m1 lc1 + m2 l1) g sin theta1 + phi2
 *        = -((0.5 theta2dot + theta1dot) theta2dot) sin theta2 + 14.7 sin theta1 + phi2
 *   theta2acc = (a + d2 / d1 phi1 - m2 l1 lc2 theta1dot^2 sin theta2 - phi2) / (m2 lc2^2 + I2 - d2^2 / d1)
 *             = (a + (d2 / d1) phi1 - 0.5 theta1dot^2 sin theta2 - phi2) / (1.25 - d2 (d2 / d1))
 *   theta1acc = -(d2 theta2acc + phi1) / d1
 * The denominator of theta2acc lies in [0.569, 1.025]: there is no singularity.
 *
 * The helpers carry the prefix acro_ (tests/test_capi_cpu.py takes a ppo_ / psyn_ / pwrap_ call at
 * the start of a header line for an exported declaration).
 */
#ifndef PPO_ACROBOT_H
#define PPO_ACROBOT_H

#include "ppo_pendulum.h"

#define ACRO_OBS_DIM 6
#define ACRO_ACT_DIM 1
#define ACRO_STATE_DIM 4
#define ACRO_MAX_STEPS 500
/*                                                  float64 value             the fp32 number            */
#define ACRO_DT 0.2f                             /* 0.2                       0.20000000298023224        */
#define ACRO_DT_HALF 0.1f                        /* 0.1                       0.10000000149011612        */
#define ACRO_DT_SIXTH 0.033333333333333333f      /* 0.03333333333333333       0.03333333507180214        */
#define ACRO_D1_0 3.5f                           /* 3.5                       exact                      */
#define ACRO_D2_0 1.25f                          /* 1.25                      exact                      */
#define ACRO_D2_C 0.5f                           /* 0.5                       exact                      */
#define ACRO_PHI2_G 4.9f                         /* 4.9 (= 0.5 * 9.8)         4.900000095367432          */
#define ACRO_PHI1_G 14.7f                        /* 14.700000000000001 (= 1.5 * 9.8) 14.699999809265137  */
#define ACRO_MAX_VEL_1 12.566370614359172f       /* 4 pi = 12.566370614359172 12.566370964050293         */
#define ACRO_MAX_VEL_2 28.274333882308138f       /* 9 pi = 28.274333882308138 28.274333953857422         */
#define ACRO_INV_TWO_PI 0.15915494309189535f     /* 1 / (2 pi)                0.15915493667125702        */
/* 2 pi = ACRO_TWO_PI_HI + ACRO_TWO_PI_LO + 1.4e-15: the fp32 number next to 2 pi (PEND_TWO_PI) and the
 * rest rounded to fp32 */
#define ACRO_TWO_PI_HI PEND_TWO_PI               /* 6.283185307179586         6.2831854820251465         */
#define ACRO_TWO_PI_LO -1.74845560007449713e-7f  /* 2 pi - ACRO_TWO_PI_HI = -1.7484556000744883e-07      */

/* x - k 2 pi with k = rint(x / 2 pi), by a two-constant Cody-Waite pair: each fmaf rounds once, after
 * its subtraction, so the result carries two roundings of values of magnitude <= pi and the 1.4e-15 k
 * the two constants leave out. It lies in [-pi - e, pi + e] with e of the order of ulp(x) (the
 * product x / 2 pi can round across a half): pend_sincos takes it as it is, and pend_wrap brings it
 * into [-pi, pi). rintf rounds to nearest even on the host and on the device (v_rndne_f32). */
PEND_FN float acro_reduce(float x) {
  PEND_NO_CONTRACT
  const float k = rintf((x * ACRO_INV_TWO_PI));
  const float r = fmaf((0.0f - k), ACRO_TWO_PI_HI, x);
  return fmaf((0.0f - k), ACRO_TWO_PI_LO, r);
}

/* the angular accelerations at (th1, th2, w1, w2) under the torque a (already clipped); the first
 * two components of the derivative are w1 and w2 themselves */
PEND_FN void acro_deriv(float th1, float th2, float w1, float w2, float a, float* acc1, float* acc2) {
  PEND_NO_CONTRACT
  float s1, c1, s2, c2;
  pend_sincos(acro_reduce(th1), &s1, &c1);
  pend_sincos(acro_reduce(th2), &s2, &c2);
  const float s12 = fmaf(s1, c2, (c1 * s2));
  const float d1 = (ACRO_D1_0 + c2);
  const float d2 = fmaf(ACRO_D2_C, c2, ACRO_D2_0);
  const float phi2 = (ACRO_PHI2_G * s12);
  const float phi1 = (fmaf(ACRO_PHI1_G, s1, phi2) - ((fmaf(0.5f, w2, w1) * w2) * s2));
  const float r = (d2 / d1);
  const float num = ((fmaf(r, phi1, a) - ((0.5f * (w1 * w1)) * s2)) - phi2);
  const float den = fmaf((0.0f - d2), r, ACRO_D2_0);
  const float a2 = (num / den);
  *acc2 = a2;
  *acc1 = (0.0f - (fmaf(d2, a2, phi1) / d1));
}

/* obs = (cos th1, sin th1, cos th2, sin th2, w1, w2) of a wrapped state; returns the termination
 * flag of that state, 1.0f | 0.0f */
PEND_FN float acro_obs(const float* s, float* obs) {
  PEND_NO_CONTRACT
  float s1, c1, s2, c2;
  pend_sincos(s[0], &s1, &c1);
  pend_sincos(s[1], &s2, &c2);
  obs[0] = c1;
  obs[1] = s1;
  obs[2] = c2;
  obs[3] = s2;
  obs[4] = s[2];
  obs[5] = s[3];
  const float c12 = fmaf(c1, c2, (0.0f - (s1 * s2)));
  return (((0.0f - c1) - c12) > 1.0f) ? 1.0f : 0.0f;
}

/* reset: every state value is 0.2 u - 0.1, u uniform in (0, 1] (so each lies in (-0.1f, 0.1f]: 0.2f
 * is exactly 2 * 0.1f) */
PEND_FN void acro_reset(const float* u, float* s) {
  PEND_NO_CONTRACT
  for (int i = 0; i < ACRO_STATE_DIM; ++i) s[i] = fmaf(0.2f, u[i], -0.1f);
}

/* One step in place on s; writes the observation and the termination flag (1.0f | 0.0f) of the new
 * state and returns the reward. The torque is clipped to [-1, 1] here, always, after whatever the
 * vector env's clip_actions did (a NaN action gives torque -1, as fminf / fmaxf give it).
 * RK4 as three passes "stage state -> derivative -> weighted sum": y is the stage's state, (dy0, dy1,
 * dy2, dy3) = (y[2], y[3], acc1, acc2) its derivative, sum = k1 + 2 k2 + 2 k3 + k4. */
PEND_FN float acro_step(float* s, float a, float* obs, float* term) {
  PEND_NO_CONTRACT
  const float u = fminf(fmaxf(a, -1.0f), 1.0f);
  float y[4], sum[4];
  acro_deriv(s[0], s[1], s[2], s[3], u, &sum[2], &sum[3]);
  sum[0] = s[2];
  sum[1] = s[3];
  y[0] = fmaf(ACRO_DT_HALF, sum[0], s[0]);
  y[1] = fmaf(ACRO_DT_HALF, sum[1], s[1]);
  y[2] = fmaf(ACRO_DT_HALF, sum[2], s[2]);
  y[3] = fmaf(ACRO_DT_HALF, sum[3], s[3]);
  for (int st = 0; st < 3; ++st) {
    /* stages 2, 3, 4: weights 2, 2, 1; the next stage's state is s + h * this derivative */
    const float w = (st < 2) ? 2.0f : 1.0f;
    const float h = (st < 1) ? ACRO_DT_HALF : ACRO_DT;
    float a1, a2;
    acro_deriv(y[0], y[1], y[2], y[3], u, &a1, &a2);
    const float d0 = y[2], d1 = y[3];
    sum[0] = fmaf(w, d0, sum[0]);
    sum[1] = fmaf(w, d1, sum[1]);
    sum[2] = fmaf(w, a1, sum[2]);
    sum[3] = fmaf(w, a2, sum[3]);
    if (st < 2) {
      y[0] = fmaf(h, d0, s[0]);
      y[1] = fmaf(h, d1, s[1]);
      y[2] = fmaf(h, a1, s[2]);
      y[3] = fmaf(h, a2, s[3]);
    }
  }
  s[0] = pend_wrap(acro_reduce(fmaf(ACRO_DT_SIXTH, sum[0], s[0])));
  s[1] = pend_wrap(acro_reduce(fmaf(ACRO_DT_SIXTH, sum[1], s[1])));
  s[2] = fminf(fmaxf(fmaf(ACRO_DT_SIXTH, sum[2], s[2]), (0.0f - ACRO_MAX_VEL_1)), ACRO_MAX_VEL_1);
  s[3] = fminf(fmaxf(fmaf(ACRO_DT_SIXTH, sum[3], s[3]), (0.0f - ACRO_MAX_VEL_2)), ACRO_MAX_VEL_2);
  const float t = acro_obs(s, obs);
  *term = t;
  return (t != 0.0f) ? 0.0f : -1.0f;
}

#endif
