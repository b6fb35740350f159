// ppo_dist.hpp — the policy distributions and the PPO loss, one text of each formula. Callers: k_act2,
// k_act4 and the tanh-Normal k_act3 (act), k_rollout / k_beta_logp / k_rollout4's log-prob (rollout), k_fwdbwd,
// the reachable Beta branch and the surrogate of k_upd / k_upd32, k_upd2's surrogate (update), k_carla_head_bwd
// and parts of k_carla_head / k_carla_tail. Not every copy could move here: a call is the parent's arithmetic
// only where the compiler contracts and allocates the inlined body as it did the parent's text, and the
// LayerNorm-Beta k_act3, k_eval, most of upd_loss and of k_upd2 keep their own text for measured reasons
// (DESIGN §4a lists each site; each carries a comment). Masking of rows past the batch stays with the callers.
#pragma once

#include "ppo_agent.hpp"
#include "ppo_kernels.hpp"

// ------------------------------------------------------------------------------------------
// Special functions of one Beta concentration: (lgamma, digamma, trigamma). Three arithmetics, kept
// apart because merging them changes bits: the Stirling one below, the device library's,
// and CaRL's opaque_ form in ppo_carla_tail.hip.
// ------------------------------------------------------------------------------------------
struct Sf3 {
  float lg, dg, tg;
};
struct SfStirling {  // one shared shift + Stirling series (k_upd / k_upd32, k_rollout, k_beta_logp)
  static PPO_DEV Sf3 at(float x) {
    Sf3 r;
    lgamma_digamma_trigamma(x, r.lg, r.dg, r.tg);
    return r;
  }
};
// The device-library arithmetic (lgammaf, digammaf_, trigammaf_: k_act2, k_fwdbwd, k_carla_head_bwd) has no
// provider: its sites need two of the three values, or all three in an order of their own, and
// call the functions directly.

// ------------------------------------------------------------------------------------------
// Beta head on [lo, hi] (rl_utils.h:87-132; Dirichlet log_prob :64-72, entropy :73-80)
// ------------------------------------------------------------------------------------------
// The Beta head's per-block work items, shared by k_act3 and the persistent kernels: item idx of a
// block's R x A x 2 is (row r, action ai, which: 0 alpha | 1 beta); its concentration comes from head
// ai + which * A, and db is the base of its gamma sample's Philox draws.
struct BetaItem {
  int which, r, ai;
  uint32_t db;
};
PPO_DEV BetaItem beta_item(int idx, int A) {
  const int which = idx & 1, ra = idx >> 1, r = ra / A, ai = ra - r * A;
  return BetaItem{which, r, ai, 0x10000u + (uint32_t)(ai * 2 + which) * 64u};
}
// the action on [lo, hi] from the Beta sample (or mean, or mode) on [0, 1]
PPO_DEV float beta_action(float s01, float lo, float hi) { return (s01 - 0.0f) / (1.0f - 0.0f) * (hi - lo) + lo; }
// a given action on [lo, hi] back on [0, 1] (scale_action), clamped off the density's poles
PPO_DEV float beta_unit_from_action(float av, float lo, float hi) {
  const float s = (av - lo) / (hi - lo) * (1.0f - 0.0f) + 0.0f;
  return fminf(fmaxf(s, 1e-7f), 1.0f + 1e-7f);
}
// the value on [0, 1] by mode: the given one, the mean, roach_deterministic, or the sample from the
// two gamma draws (PPO_CARLA_* are the same four values)
PPO_DEV float beta_unit(int mode, float al, float be, float ga, float gb, float given) {
  if (mode == PPO_GIVEN) return given;
  if (mode == PPO_MEAN) return al / (al + be);
  if (mode == PPO_ROACH) return beta_roach01(al, be);
  return beta_sample01(ga, gb);
}
// one action's log-prob and entropy terms from the lgamma / digamma of alpha, beta and alpha + beta
PPO_DEV float beta_logp_term(float al, float be, float s, float lga, float lgb, float lgab) {
  return xlogyf_(al - 1.0f, s) + xlogyf_(be - 1.0f, 1.0f - s) + (lgab - (lga + lgb));
}
PPO_DEV float beta_ent_term(float al, float be, float lga, float lgb, float lgab, float psa, float psb, float psab) {
  const float ab = al + be;
  return (lga + lgb) - lgab - (2.0f - ab) * psab - ((al - 1.0f) * psa + (be - 1.0f) * psb);
}
// d log-prob / d (alpha, beta) and d entropy / d (alpha, beta) of one action. xlogy's backward at a
// concentration of exactly 1 is 0, not log(s).
struct BetaGrad {
  float dla, dlb, dea, deb;
};
PPO_DEV BetaGrad beta_grad(float al, float be, float s, float psa, float psb, float psab, float ta, float tb,
                           float tab) {
  const float ab = al + be;
  BetaGrad g;
  g.dla = ((al - 1.0f) != 0.0f ? logf(s) : 0.0f) + psab - psa;
  g.dea = (ab - 2.0f) * tab - (al - 1.0f) * ta;
  g.dlb = ((be - 1.0f) != 0.0f ? logf(1.0f - s) : 0.0f) + psab - psb;
  g.deb = (ab - 2.0f) * tab - (be - 1.0f) * tb;
  return g;
}

// ------------------------------------------------------------------------------------------
// Normal head (rl_utils.h:34-45)
// ------------------------------------------------------------------------------------------
static constexpr float kLz = 0.91893853320467274178f;   // log(sqrt(2 pi))  (rl_utils.h:20)
static constexpr float kEntC = 1.4189385332046727418f;  // 0.5 + 0.5 log(2 pi) (rl_utils.h:44)
// the standard-normal draw of (env, step, action ai): actions 2 k and 2 k + 1 share Philox draw k
PPO_DEV float normal_z(SampleKey key, long env, long step, int ai) {
  uint32_t rr[4];
  philox_draw(key, env, step, (uint32_t)(ai >> 1), rr);
  float z0, z1;
  box_muller(rr[0], rr[1], z0, z1);
  return (ai & 1) ? z1 : z0;
}
PPO_DEV float normal_logp_term(float act, float mu, float var, float lsd) {
  const float d = act - mu;
  return -(d * d) / (2.0f * var) - lsd - kLz;
}
PPO_DEV float normal_ent_term(float lsd) { return kEntC + lsd; }
// d log-prob / d mu and d log-prob / d logstd of one action, d = action - mu
struct NormalGrad {
  float dmu, dls;
};
PPO_DEV NormalGrad normal_grad(float d, float var) { return NormalGrad{d / var, d * d / var - 1.0f}; }

// ------------------------------------------------------------------------------------------
// PPO loss per row (ppo:497-527, ac:815-875)
// ------------------------------------------------------------------------------------------
// clipped surrogate (ppo:497-513): d loss / d log-prob, d loss / d entropy and the row's terms of the
// policy loss, old_approx_kl, approx_kl and clipfrac. Ties of max(pg1, pg2) split the gradient (ATen
// maximum backward).
struct PpoSurrogate {
  float g_logp, g_ent, pg, okl, kl, clipfrac;
};
PPO_DEV PpoSurrogate ppo_surrogate(float lp, float oldlp, float adv, int norm_adv, float adv_mean, float adv_std,
                                   float clip, float inv_m, float ent_coef) {
  const float c = clip;
  const float logratio = lp - oldlp;
  const float ratio = expf(logratio);
  float an = adv;
  if (norm_adv) an = (an - adv_mean) / (adv_std + 1e-8f);
  const float rc = fminf(fmaxf(ratio, 1.0f - c), 1.0f + c);
  const float pg1 = -an * ratio, pg2 = -an * rc;
  const float w1 = pg1 > pg2 ? 1.0f : (pg1 == pg2 ? 0.5f : 0.0f);
  const float inr = (ratio >= 1.0f - c && ratio <= 1.0f + c) ? 1.0f : 0.0f;
  PpoSurrogate r;
  r.g_logp = inv_m * (w1 * (-an) + (1.0f - w1) * (-an) * inr) * ratio;
  r.g_ent = -ent_coef * inv_m;
  r.pg = fmaxf(pg1, pg2);
  r.okl = -logratio;
  r.kl = (ratio - 1.0f) - logratio;
  r.clipfrac = fabsf(ratio - 1.0f) > c ? 1.0f : 0.0f;
  return r;
}
// value loss (ppo:515-527), clipped or plain: d loss / d value and the row's term (before the 0.5)
struct PpoValueLoss {
  float g_v, term;
};
PPO_DEV PpoValueLoss ppo_value_loss(float v, float ret, float old_v, float clip, int clip_vloss, float vf_coef,
                                    float inv_m) {
  const float c = clip;
  PpoValueLoss r;
  if (clip_vloss) {
    const float vu = (v - ret) * (v - ret);
    const float dv = v - old_v;
    const float vcl = old_v + fminf(fmaxf(dv, -c), c);
    const float vc = (vcl - ret) * (vcl - ret);
    r.term = fmaxf(vu, vc);
    const float w1 = vu > vc ? 1.0f : (vu == vc ? 0.5f : 0.0f);
    const float inr = (dv >= -c && dv <= c) ? 1.0f : 0.0f;
    r.g_v = 0.5f * vf_coef * inv_m * (w1 * 2.0f * (v - ret) + (1.0f - w1) * 2.0f * (vcl - ret) * inr);
  } else {
    r.term = (v - ret) * (v - ret);
    r.g_v = 0.5f * vf_coef * inv_m * 2.0f * (v - ret);
  }
  return r;
}
