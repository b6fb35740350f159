/*
 * ppo_cheetah.h — the arithmetic of the synthetic HalfCheetah-shaped env (ppo_synth_env.h), shared by
 * the host env (ppo.cpp_amd/gymcpp/synthetic_cheetah.h) and the device env kernels (ppo_kernels.hip,
 * ppo_rollout.hip, ppo_eval.hip). Plain C. The oracle (oracle/ppo_oracle.c) restates these formulas on
 * its own and does not include this file: it is the independent check.
 *
 * The env exists at any (O, A), so the header holds the per-element pieces and each user walks the
 * state its own way (one lane per element, lane groups, a host loop):
 *   reset   q_i  = 0.1 (2 u_i - 1), u_i the uniform of draw i of the env's reset stream
 *   step    q'_i = fma(0.9, q_i, fma(0.1, a_(i mod A), 0.05 q_(i+1 mod O)))
 *   reward  (q'_0 - q_0) / 0.05 - sum_k (0.1 a_k) a_k
 *   truncation after CHEE_MAX_STEPS steps; the env never terminates
 * The actions are the clipped ones (clip_actions): the clip stays with the caller.
 *
 * Host and device results are bit-identical: fp32 only, every fused multiply-add written as fmaf,
 * everything else with explicit parentheses and contraction off (host: -ffp-contract=off; device: the
 * pragma below).
 *
 * The helpers carry the prefix chee_ (tests/test_capi_cpu.py takes a ppo_ / psyn_ / pwrap_ call at
 * the start of a header line for an exported declaration).
 */
#ifndef PPO_CHEETAH_H
#define PPO_CHEETAH_H

#include <math.h>

#if defined(__HIPCC__)
#define CHEE_FN static inline __host__ __device__
#else
#define CHEE_FN static inline
#endif
#if defined(__clang__)
#define CHEE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CHEE_NO_CONTRACT
#endif

#define CHEE_MAX_STEPS 1000
/* second key word of the reset stream: Philox4x32-10 keyed (env seed, CHEE_RESET_KEY), counter
 * (reset number, i, 0, 0) for draw i; the first output word makes the uniform */
#define CHEE_RESET_KEY 0x5EED5EEDu

/* state element i of a reset from its uniform u in (0, 1] */
CHEE_FN float chee_reset_value(float u) {
  CHEE_NO_CONTRACT
  return (0.1f * ((2.0f * u) - 1.0f));
}

/* q'_i from q_i, the clipped action a_(i mod A) and the old q_(i+1 mod O) */
CHEE_FN float chee_next_q(float qi, float a, float q_next) {
  CHEE_NO_CONTRACT
  return fmaf(0.9f, qi, fmaf(0.1f, a, (0.05f * q_next)));
}

/* the control cost, one clipped action at a time, from 0 and in the order k = 0 .. A-1 */
CHEE_FN float chee_ctrl_add(float ctrl, float ak) {
  CHEE_NO_CONTRACT
  return (ctrl + ((0.1f * ak) * ak));
}

/* the reward from element 0 after and before the step and the summed control cost */
CHEE_FN float chee_reward_ctrl(float q0_new, float q0_old, float ctrl) {
  CHEE_NO_CONTRACT
  return (((q0_new - q0_old) / 0.05f) - ctrl);
}

/* the reward from the A clipped actions */
CHEE_FN float chee_reward(float q0_new, float q0_old, const float* ac, int A) {
  float ctrl = 0.0f;
  for (int k = 0; k < A; ++k) ctrl = chee_ctrl_add(ctrl, ac[k]);
  return chee_reward_ctrl(q0_new, q0_old, ctrl);
}

#endif
