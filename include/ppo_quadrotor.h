/*
 * ppo_quadrotor.h — the arithmetic of QuadrotorHover-v0, a rigid-body quadrotor in "+"
 * configuration that hovers at the origin: O = 18, A = 4, it terminates (|p|^2 > 9) and truncates
 * (500 steps). It is not a simulator's quadrotor and not a Gymnasium env: the task is this project's
 * own, the textbook Newton-Euler equations with a unit quaternion, per-rotor thrusts, linear drag and
 * rate damping, semi-implicit Euler in two substeps per env step. No ground, no motor dynamics.
 * Shared by the host env (ppo.cpp_amd/gymcpp/quadrotor.h), the device env kernels (ppo_kernels.hip,
 * ppo_rollout.hip, ppo_eval.hip) and the test driver (tests/native/quadrotor_driver.cpp). Plain C.
 *
 * Host and device results are bit-identical, by the rules of ppo_pendulum.h: fp32 only, every fused
 * multiply-add written as fmaf, everything else with explicit parentheses and contraction off. There
 * is no trigonometric function anywhere in the task. The divisions and the sqrtf are plain and
 * correctly rounded on the host and on the device (hipcc's default; no reciprocal or rsqrt
 * approximation, no fast-math).
 *
 * The state is s = (p[3], v[3], q = (w, x, y, z), omega[3]): 13 floats. The observation, on the new
 * state, is (p, R(q) row-major, v, omega): 18 floats. The rotors sit at +x, +y, -x, -y (0..3);
 * rotor i pushes f_i = 1/2 (clip(a_i, -1, 1) + 1) f_max along the body's z axis, f_max = g / 2, so
 * a = 0 hovers. F = sum f_i, tau_x = d (f1 - f3), tau_y = d (f2 - f0),
 * tau_z = kappa (f0 - f1 + f2 - f3). One substep, in this order: R = R(q);
 * vdot = F R e_z - g e_z - c_d v; the Euler equations with the damping c_w omega;
 * omega <- clip(omega + dt omegadot, +-32); v <- v + dt vdot; p <- p + dt v (new v);
 * q <- normalise(q + dt / 2 q (x) (0, omega)) (new omega).
 * Reward on the new state, on the terminating step too: r_p = 1 / (1 + |p|^2),
 * r = r_p + r_p (1 / (1 + (1 - R33)^2) + 1 / (1 + |omega|^2)), in (0, 3]. The episode terminates when
 * |p|^2 > 9, compared in fp32 on the new state; truncation after 500 steps is the caller's.
 *
 * One departure from the textbook integrator: the body rates are clipped to +-32 rad/s after each
 * substep, so that no state value can run away between a termination test and the reset.
 *
 * Constants: float64 value, then the fp32 value used:
 *   g = 9.81                       9.8100004196166992
 *   f_max = g / 2 = 4.905          4.9050002098083496
 *   d = 0.1                        0.10000000149011612    arm
 *   kappa = 0.02                   0.019999999552965164   yaw coefficient
 *   I_xx = I_yy = 0.01             0.0099999997764825821
 *   I_zz = 0.02                    0.019999999552965164
 *   I_zz - I_yy = 0.01             0.0099999997764825821  (I_xx - I_zz is its negative)
 *   c_d = 0.1                      0.10000000149011612    linear drag
 *   c_w = 0.002                    0.0020000000949949026  rate damping
 *   dt = 0.01                      0.0099999997764825821  substep
 *   dt / 2 = 0.005                 0.004999999888241291
 * with m = 1.
 *
 * The helpers carry the prefix quad_ (tests/test_capi_cpu.py takes a ppo_ / psyn_ / pwrap_ call at
 * the start of a header line for an exported declaration).
 */
#ifndef PPO_QUADROTOR_H
#define PPO_QUADROTOR_H

#include "ppo_pendulum.h"

#define QUAD_OBS_DIM 18
#define QUAD_ACT_DIM 4
#define QUAD_STATE_DIM 13
#define QUAD_RESET_DRAWS 12
#define QUAD_MAX_STEPS 500
#define QUAD_SUBSTEPS 2
#define QUAD_G 9.81f
#define QUAD_FMAX 4.905f
#define QUAD_ARM 0.1f
#define QUAD_KAPPA 0.02f
#define QUAD_IXX 0.01f
#define QUAD_IZZ 0.02f
#define QUAD_IZY 0.01f /* I_zz - I_yy = -(I_xx - I_zz) */
#define QUAD_CD 0.1f
#define QUAD_CW 0.002f
#define QUAD_DT 0.01f
#define QUAD_HALF_DT 0.005f
#define QUAD_MAX_RATE 32.0f
#define QUAD_TERM_P2 9.0f

/* R(q) row-major from a unit quaternion (w, x, y, z) */
PEND_FN void quad_rot(float w, float x, float y, float z, float* R) {
  PEND_NO_CONTRACT
  R[0] = fmaf(-2.0f, fmaf(y, y, (z * z)), 1.0f);
  R[1] = (2.0f * fmaf(x, y, (0.0f - (w * z))));
  R[2] = (2.0f * fmaf(x, z, (w * y)));
  R[3] = (2.0f * fmaf(x, y, (w * z)));
  R[4] = fmaf(-2.0f, fmaf(x, x, (z * z)), 1.0f);
  R[5] = (2.0f * fmaf(y, z, (0.0f - (w * x))));
  R[6] = (2.0f * fmaf(x, z, (0.0f - (w * y))));
  R[7] = (2.0f * fmaf(y, z, (w * x)));
  R[8] = fmaf(-2.0f, fmaf(x, x, (y * y)), 1.0f);
}

/* obs = (p, R row-major, v, omega) of the state s. obs may not overlap s. */
PEND_FN void quad_obs(const float* s, float* obs) {
  quad_rot(s[6], s[7], s[8], s[9], obs + 3);
  for (int i = 0; i < 3; ++i) {
    obs[i] = s[i];
    obs[12 + i] = s[3 + i];
    obs[15 + i] = s[10 + i];
  }
}

/* reset from twelve uniforms in (0, 1], in the order p, v, e, omega: p = 2 u - 1, v = u - 0.5,
 * q = normalise(1, e) with e = 0.4 u - 0.2, omega = u - 0.5 */
PEND_FN void quad_reset(const float* u, float* s) {
  PEND_NO_CONTRACT
  for (int i = 0; i < 3; ++i) {
    s[i] = fmaf(2.0f, u[i], -1.0f);
    s[3 + i] = (u[3 + i] - 0.5f);
    s[10 + i] = (u[9 + i] - 0.5f);
  }
  const float ex = fmaf(0.4f, u[6], -0.2f), ey = fmaf(0.4f, u[7], -0.2f), ez = fmaf(0.4f, u[8], -0.2f);
  const float n = sqrtf(fmaf(ex, ex, fmaf(ey, ey, fmaf(ez, ez, 1.0f))));
  s[6] = (1.0f / n);
  s[7] = (ex / n);
  s[8] = (ey / n);
  s[9] = (ez / n);
}

/* one semi-implicit substep under the total thrust F and the body torques (tx, ty, tz) */
PEND_FN void quad_substep(float* s, float F, float tx, float ty, float tz) {
  PEND_NO_CONTRACT
  const float qw = s[6], qx = s[7], qy = s[8], qz = s[9];
  const float wx = s[10], wy = s[11], wz = s[12];
  /* the third column of R(q) */
  const float r13 = (2.0f * fmaf(qx, qz, (qw * qy)));
  const float r23 = (2.0f * fmaf(qy, qz, (0.0f - (qw * qx))));
  const float r33 = fmaf(-2.0f, fmaf(qx, qx, (qy * qy)), 1.0f);
  const float ax = fmaf((0.0f - QUAD_CD), s[3], (F * r13));
  const float ay = fmaf((0.0f - QUAD_CD), s[4], (F * r23));
  const float az = fmaf((0.0f - QUAD_CD), s[5], fmaf(F, r33, (0.0f - QUAD_G)));
  const float dwx = (fmaf((0.0f - QUAD_CW), wx, fmaf((0.0f - QUAD_IZY), (wy * wz), tx)) / QUAD_IXX);
  const float dwy = (fmaf((0.0f - QUAD_CW), wy, fmaf(QUAD_IZY, (wz * wx), ty)) / QUAD_IXX);
  const float dwz = (fmaf((0.0f - QUAD_CW), wz, tz) / QUAD_IZZ);
  const float nwx = fminf(fmaxf(fmaf(QUAD_DT, dwx, wx), (0.0f - QUAD_MAX_RATE)), QUAD_MAX_RATE);
  const float nwy = fminf(fmaxf(fmaf(QUAD_DT, dwy, wy), (0.0f - QUAD_MAX_RATE)), QUAD_MAX_RATE);
  const float nwz = fminf(fmaxf(fmaf(QUAD_DT, dwz, wz), (0.0f - QUAD_MAX_RATE)), QUAD_MAX_RATE);
  const float nvx = fmaf(QUAD_DT, ax, s[3]);
  const float nvy = fmaf(QUAD_DT, ay, s[4]);
  const float nvz = fmaf(QUAD_DT, az, s[5]);
  s[0] = fmaf(QUAD_DT, nvx, s[0]);
  s[1] = fmaf(QUAD_DT, nvy, s[1]);
  s[2] = fmaf(QUAD_DT, nvz, s[2]);
  s[3] = nvx;
  s[4] = nvy;
  s[5] = nvz;
  /* q (x) (0, omega), with the new omega */
  const float ew = (0.0f - fmaf(qx, nwx, fmaf(qy, nwy, (qz * nwz))));
  const float ex = fmaf(qw, nwx, fmaf(qy, nwz, (0.0f - (qz * nwy))));
  const float ey = fmaf(qw, nwy, fmaf(qz, nwx, (0.0f - (qx * nwz))));
  const float ez = fmaf(qw, nwz, fmaf(qx, nwy, (0.0f - (qy * nwx))));
  const float uw = fmaf(QUAD_HALF_DT, ew, qw);
  const float ux = fmaf(QUAD_HALF_DT, ex, qx);
  const float uy = fmaf(QUAD_HALF_DT, ey, qy);
  const float uz = fmaf(QUAD_HALF_DT, ez, qz);
  const float n = sqrtf(fmaf(uw, uw, fmaf(ux, ux, fmaf(uy, uy, (uz * uz)))));
  s[6] = (uw / n);
  s[7] = (ux / n);
  s[8] = (uy / n);
  s[9] = (uz / n);
  s[10] = nwx;
  s[11] = nwy;
  s[12] = nwz;
}

/* One env step in place on s; writes the observation of the new state and the termination flag
 * (1.0f | 0.0f) and returns the reward. The four actions are clipped to [-1, 1] here, always, after
 * whatever the vector env's clip_actions did (a NaN action gives -1, as fminf / fmaxf give it).
 * obs may not overlap s. */
PEND_FN float quad_step(float* s, const float* a, float* obs, float* term) {
  PEND_NO_CONTRACT
  const float f0 = ((0.5f * (fminf(fmaxf(a[0], -1.0f), 1.0f) + 1.0f)) * QUAD_FMAX);
  const float f1 = ((0.5f * (fminf(fmaxf(a[1], -1.0f), 1.0f) + 1.0f)) * QUAD_FMAX);
  const float f2 = ((0.5f * (fminf(fmaxf(a[2], -1.0f), 1.0f) + 1.0f)) * QUAD_FMAX);
  const float f3 = ((0.5f * (fminf(fmaxf(a[3], -1.0f), 1.0f) + 1.0f)) * QUAD_FMAX);
  const float F = ((f0 + f1) + (f2 + f3));
  const float tx = (QUAD_ARM * (f1 - f3));
  const float ty = (QUAD_ARM * (f2 - f0));
  const float tz = (QUAD_KAPPA * ((f0 - f1) + (f2 - f3)));
  for (int k = 0; k < QUAD_SUBSTEPS; ++k) quad_substep(s, F, tx, ty, tz);
  quad_obs(s, obs);
  const float p2 = fmaf(s[0], s[0], fmaf(s[1], s[1], (s[2] * s[2])));
  const float w2 = fmaf(s[10], s[10], fmaf(s[11], s[11], (s[12] * s[12])));
  const float up = (1.0f - obs[11]); /* 1 - R33 */
  const float rp = (1.0f / (1.0f + p2));
  const float ru = (1.0f / fmaf(up, up, 1.0f));
  const float rw = (1.0f / (1.0f + w2));
  *term = (p2 > QUAD_TERM_P2) ? 1.0f : 0.0f;
  return fmaf(rp, (ru + rw), rp);
}

#endif
