// ppo_rollout_common.hpp — building blocks of the persistent kernels of the 256-wide LayerNorm-Beta
// agent: k_rollout / k_values (ppo_rollout.hip) and k_eval (ppo_eval.hip). LDS geometry, the per-env
// scalar slots, their load / store (env_slots_load / env_slots_store), the episode contract on them
// (ev_autoreset, ev_step_account) and the env step on them (env_lane_step for a kind with a DevEnv,
// chee_lanes_step for the cheetah; k_rollout_v uses them too, k_rollout4 env_lane_step), the staged small
// parameters, the register-resident weight slices and one trunk forward for the rows in XS. Kernels
// that use them in the same order produce bitwise identical results (and bitwise k_act3's, whose
// blocks of ppo_act_common.hpp they are built from).
//
// A translation unit of the diagnostic stamps build defines ROLL_STAMP / RDBG / kRdbgEnv before it
// includes this file; without them the hooks compile to nothing.
#pragma once

#include "ppo_act_common.hpp"
#include "ppo_env_kinds.hpp"

#include <type_traits>

#ifndef ROLL_STAMP
#define ROLL_STAMP(t, k) do {} while (0)
#endif

namespace {

using namespace act;

constexpr int kRows = 16;  // envs (rows) per workgroup

template <int NTO, int NHT, int ROWS = kRows>
struct RollGeo {
  static constexpr int kRows = ROWS;  // rows per pass (16: the rollout's env block; 32: k_values)
  static constexpr int H = 256, OP = NTO * 16, NHP = 16 * NHT;
  static constexpr int LDX = ((OP + 63) / 64) * 64 + 4;
  static constexpr int LDH = H + 4;
  static constexpr int LDP = NHP + 4;
  static constexpr int LDQ = OP + 1;                           // env state / obs rows (O <= OP)
  static constexpr int NSP = 6 * H + NHP * H;
  static constexpr int oXS = 0;
  static constexpr int oHB = oXS + kRows * LDX;
  static constexpr int oSP = oHB + kRows * LDH;
  static constexpr int oHBIAS = oSP + NSP;
  static constexpr int oRED = oHBIAS + NHP;
  static constexpr int oHP = oRED + 2 * kActWaves * kRows;
  static constexpr int oPRE = oHP + kActWaves * NHP * kRows;
  static constexpr int oXO = oPRE + kRows * LDP;               // agent input obs of the current step
  static constexpr int oQ = oXO + kRows * LDQ;                 // env state q
  static constexpr int oNRM = oQ + kRows * LDQ;                // obs mean | std (OP each)
  static constexpr int oACT = oNRM + 2 * OP;                   // actions [16][24]
  static constexpr int oENV = oACT + kRows * 24;               // per-env scalars, 16 x 16
  static constexpr int total = oENV + 16 * kRows;
  // distribution scratch in the XS / HB region (dead after layer 2), as in k_act3
  static constexpr int oITM = 0;
  static constexpr int oLP = oITM + kRows * 24 * 2 * 4;
  static_assert(oLP + kRows * 24 * 2 <= oSP, "distribution scratch must fit in the XS/HB region");
  // staged param vectors inside SP (as ActGeo)
  static constexpr int sB1 = 0, sG1 = H, sBE1 = 2 * H, sB2 = 3 * H, sG2 = 4 * H, sBE2 = 5 * H, sW3 = 6 * H;
};

// per-env scalar slots in the oENV region
// (the wrapper chain's per-env scalars: obs count, return accumulator, reward mean / var / count)
enum { EV_DONE = 0, EV_AR, EV_T, EV_RSEED, EV_RCOUNT, EV_EPR, EV_EPL, EV_FR, EV_FL, EV_FC,
       EV_WOC, EV_WRA, EV_WRM, EV_WRV, EV_WRC, EV_NSLOT };

// The ten per-env scalars and the q / obs rows of a workgroup's R envs [row0, row0 + R) between global
// memory and LDS, by all NT threads: the prologue and the epilogue of a persistent kernel. obs is the
// agent's next input ([E][O]); next_done may be null (the evaluation has none: EV_DONE is not used).
// A row past the last env E - 1 loads zero rows and env E - 1's scalars, and is not stored. The
// caller's barrier follows the load. (k_rollout4 keeps its own passes, which also move the wrapper
// chain's rows and slots: DESIGN 5u.)
template <int R, int NT>
PPO_DEV void env_slots_load(float* EV, float* XO, float* Q, int ldq, const SynthArgs& sv, const float* obs,
                            const float* next_done, int row0, int E, int O, int tid) {
  int* EVI = reinterpret_cast<int*>(EV);
  for (int idx = tid; idx < R * O; idx += NT) {
    const int r = idx / O, f = idx - r * O, e = row0 + r;
    XO[r * ldq + f] = e < E ? obs[(long)e * O + f] : 0.0f;
    Q[r * ldq + f] = e < E ? sv.q[(long)e * O + f] : 0.0f;
  }
  if (tid < R) {
    const int e = min(row0 + tid, E - 1);
    if (next_done) EV[EV_DONE * R + tid] = next_done[e];
    EVI[EV_AR * R + tid] = sv.autoreset[e];
    EVI[EV_T * R + tid] = sv.t[e];
    EVI[EV_RSEED * R + tid] = (int)sv.rseed[e];
    EVI[EV_RCOUNT * R + tid] = (int)sv.rcount[e];
    EV[EV_EPR * R + tid] = sv.ep_ret[e];
    EVI[EV_EPL * R + tid] = sv.ep_len[e];
    EV[EV_FR * R + tid] = sv.fin_ret[e];
    EV[EV_FL * R + tid] = sv.fin_len[e];
    EV[EV_FC * R + tid] = sv.fin_cnt[e];
  }
}
template <int R, int NT>
PPO_DEV void env_slots_store(const float* EV, const float* XO, const float* Q, int ldq, const SynthArgs& sv, float* obs,
                             float* next_done, int row0, int E, int O, int tid) {
  const int* EVI = reinterpret_cast<const int*>(EV);
  for (int idx = tid; idx < R * O; idx += NT) {
    const int r = idx / O, f = idx - r * O, e = row0 + r;
    if (e < E) {
      obs[(long)e * O + f] = XO[r * ldq + f];
      sv.q[(long)e * O + f] = Q[r * ldq + f];
    }
  }
  if (tid < R && row0 + tid < E) {
    const int e = row0 + tid;
    if (next_done) next_done[e] = EV[EV_DONE * R + tid];
    sv.autoreset[e] = EVI[EV_AR * R + tid];
    sv.t[e] = EVI[EV_T * R + tid];
    sv.rseed[e] = (uint32_t)EVI[EV_RSEED * R + tid];
    sv.rcount[e] = (uint32_t)EVI[EV_RCOUNT * R + tid];
    sv.ep_ret[e] = EV[EV_EPR * R + tid];
    sv.ep_len[e] = EVI[EV_EPL * R + tid];
    sv.fin_ret[e] = EV[EV_FR * R + tid];
    sv.fin_len[e] = EV[EV_FL * R + tid];
    sv.fin_cnt[e] = EV[EV_FC * R + tid];
  }
}

// The episode contract on env r's EV slots (R envs per workgroup), by one lane of the env's group:
//   * an env whose episode finished (EV_AR) resets on the next step: reward 0, not finished, a new
//     episode from reset number EV_RCOUNT of its Philox stream, the episode counters cleared
//     (ev_autoreset, after the draws of reset number rc)
//   * otherwise the step; fin = terminated or truncated (EV_T reached max_steps); the step joins the
//     running episode (EV_EPR, EV_EPL), a finished episode the totals (EV_FR, EV_FL, EV_FC), and EV_AR
//     carries fin to the next step (ev_step_account, from the step's reward and termination flag)
// The caller does its own part with the outcome: the rollout's reward and EV_DONE stores, the wrapper
// chain (term, not fin, goes to NormalizeReward), the evaluation's episode event.
struct EnvLaneOut {
  float reward, term;  // term: 1.0f when the step terminated the episode (never on truncation)
  bool fin, reset;
  float epr;           // the episode's return and length up to this step (set when !reset)
  int epl;
};
template <int R>
PPO_DEV void ev_autoreset(float* EV, int r, uint32_t rc) {
  int* EVI = reinterpret_cast<int*>(EV);
  EVI[EV_RCOUNT * R + r] = (int)(rc + 1);
  EVI[EV_T * R + r] = 0;
  EV[EV_EPR * R + r] = 0.0f;
  EVI[EV_EPL * R + r] = 0;
  EVI[EV_AR * R + r] = 0;
}
template <int R>
PPO_DEV void ev_step_account(float* EV, int r, int max_steps, EnvLaneOut& out) {
#pragma clang fp contract(off)
  int* EVI = reinterpret_cast<int*>(EV);
  const int tt = EVI[EV_T * R + r] + 1;
  EVI[EV_T * R + r] = tt;
  out.fin = (out.term != 0.0f) || tt >= max_steps;  // done = terminated or truncated
  out.epr = (EV[EV_EPR * R + r] + out.reward);
  EV[EV_EPR * R + r] = out.epr;
  out.epl = EVI[EV_EPL * R + r] + 1;
  EVI[EV_EPL * R + r] = out.epl;
  if (out.fin) {
    EV[EV_FR * R + r] += out.epr;
    EV[EV_FL * R + r] += (float)out.epl;
    EV[EV_FC * R + r] += 1.0f;
  }
  EVI[EV_AR * R + r] = out.fin ? 1 : 0;
}

// One env step of a kind with a DevEnv, by lane 0 of the env's lane group in a persistent kernel: the
// autoreset or the step from the env's clipped actions, and the episode contract. Leaves the state in
// q and the raw observation in xo (the env's LDS rows).
template <int KIND, int R>
PPO_DEV EnvLaneOut env_lane_step(float* EV, int r, float* q, float* xo, const float* act_row, float lo, float hi) {
#pragma clang fp contract(off)
  using D = DevEnv<KIND>;
  int* EVI = reinterpret_cast<int*>(EV);
  EnvLaneOut out{0.0f, 0.0f, false, EVI[EV_AR * R + r] != 0, 0.0f, 0};
  float sreg[D::IN_PLACE ? 1 : D::S], oreg[D::IN_PLACE ? 1 : D::O];
  float* s = D::IN_PLACE ? q : sreg;
  float* o = D::IN_PLACE ? xo : oreg;
  if (out.reset) {
    const uint32_t rs = (uint32_t)EVI[EV_RSEED * R + r], rc = (uint32_t)EVI[EV_RCOUNT * R + r];
    D::reset(rc, rs, s, o);
    ev_autoreset<R>(EV, r, rc);
  } else {
    if constexpr (!D::IN_PLACE) {
#pragma unroll
      for (int i = 0; i < D::S; ++i) s[i] = q[i];
    }
    float ac[D::A];
#pragma unroll
    for (int k = 0; k < D::A; ++k) ac[k] = fminf(fmaxf(act_row[k], lo), hi);
    out.reward = D::step(s, ac, o, &out.term);
    ev_step_account<R>(EV, r, D::MAX_STEPS, out);
  }
  if constexpr (!D::IN_PLACE) {
#pragma unroll
    for (int i = 0; i < D::S; ++i) q[i] = s[i];
#pragma unroll
    for (int i = 0; i < D::O; ++i) xo[i] = o[i];
  }
  return out;
}

// The synthetic cheetah's step of env r, spread over the env's 32 lanes (lane i0 takes the elements
// i0, i0 + 32, ... of the O <= 32 NCH) on the env's LDS rows, called by all 32 lanes of a live env:
// the autoreset draw or the step (k_synth_step / k_synth_step_wide arithmetic: every old q is in
// registers before any write), and on lane 0 the reward, the episode contract and then lane0(outcome),
// the caller's own part, inside the branch taken (a reset's outcome is constants there).
template <int R, int NCH, typename F>
PPO_DEV void chee_lanes_step(float* EV, int r, int i0, int O, int A, float* q, float* xo, const float* ar, float lo,
                             float hi, F&& lane0) {
  int* EVI = reinterpret_cast<int*>(EV);
  EnvLaneOut out{0.0f, 0.0f, false, EVI[EV_AR * R + r] != 0, 0.0f, 0};
  if (out.reset) {
    const uint32_t rs = (uint32_t)EVI[EV_RSEED * R + r], rc = (uint32_t)EVI[EV_RCOUNT * R + r];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int i = 32 * c + i0;
      if (i < O) {
        const float v = chee_reset_elem(rc, rs, i);
        q[i] = v;
        xo[i] = v;
      }
    }
    if (i0 == 0) {
      ev_autoreset<R>(EV, r, rc);
      lane0(out);
    }
  } else {
    float qo[NCH], qn[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int i = 32 * c + i0;
      qo[c] = i < O ? q[i] : 0.0f;
      qn[c] = i < O ? q[i + 1 < O ? i + 1 : 0] : 0.0f;
    }
    float q0_new = 0.0f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int i = 32 * c + i0;
      if (i < O) {
        const float nq = chee_next_q(qo[c], chee_clip(ar[i % A], lo, hi), qn[c]);
        q[i] = nq;
        xo[i] = nq;
        if (c == 0) q0_new = nq;
      }
    }
    if (i0 == 0) {
      out.reward = chee_reward_clip(q0_new, qo[0], ar, A, lo, hi);
      ev_step_account<R>(EV, r, CHEE_MAX_STEPS, out);
      lane0(out);
    }
  }
}

// Env r's step in a persistent kernel whose envs have 32 lanes each (k_rollout, k_eval), called by all
// 32 lanes of a live env: the cheetah spreads its step over them, a kind with a DevEnv steps on lane 0
// from its actions ar[0..A-1]. The outcome is lane 0's.
template <int KIND, int R, int NCH, typename F>
PPO_DEV void env_lanes_step(float* EV, int r, int i0, int O, int A, float* q, float* xo, const float* ar, float lo,
                            float hi, F&& lane0) {
  if constexpr (KIND == PSYN_CHEETAH) {
    chee_lanes_step<R, NCH>(EV, r, i0, O, A, q, xo, ar, lo, hi, lane0);
  } else {
    if (i0 == 0) lane0(env_lane_step<KIND, R>(EV, r, q, xo, ar, lo, hi));
  }
}

// staged small parameters of one trunk into LDS (biases, LayerNorm affine, head rows, head biases)
template <int NHP>
PPO_DEV void stage_params(const PackedLayout& K, const TrunkDev& T, PBuf pb, int trunk, float* SP, float* HBIAS,
                          int tid) {
  constexpr int H = 256, NSP4 = (6 * H + NHP * H) / 4;
  for (int q = tid; q < NSP4; q += kActThreads) {
    const int fl = 4 * q, vec = fl / H, off = fl - vec * H;
    int src = -1;
    if (vec < 6) {
      const int base = vec == 0 ? T.b1 : vec == 1 ? T.g1 : vec == 2 ? T.be1 : vec == 3 ? T.b2 : vec == 4 ? T.g2 : T.be2;
      src = base >= 0 ? base + off : -1;
    } else {
      const int hr = act_head_row(K, trunk, vec - 6);
      src = hr >= 0 ? hr + off : -1;
    }
    *reinterpret_cast<f4*>(SP + fl) = pld4(pb, src >= 0 ? src : K.size, 0);
  }
  if (tid < NHP) {
    const int hbo = act_head_bias(K, trunk, tid);
    HBIAS[tid] = bld1f(pb, hbo >= 0 ? hbo : K.size);
  }
}

// One trunk forward for the 16 rows whose (normalised, zero-padded) inputs are in XS: layer 1,
// LayerNorm + ReLU, layer 2, LayerNorm + ReLU, heads; leaves the head pre-activations (+ bias) in
// PRE [16][LDP]. Weights: w1 / w2 register slices of this wave. Same operations, same order as
// k_act3 (LN_BETA, RT = 1).
// PRE_PASS false: stop once the per-wave head partials are in HP (after the barrier); the caller
// adds them itself (the same adds in the same order: bitwise the PRE values).
template <int NTO, int NHT, int RT = 1, bool PRE_PASS = true, typename PRE_L2 = int>
PPO_DEV void trunk_rows(const f4 (&w1)[NTO][2], const f4 (&w2)[16][2], float* lds, int nh, int tid,
                        PRE_L2 pre_l2 = 0, int stamp_t = -1) {
  (void)stamp_t;  // ROLL_STAMP step index (stamps build; -1: none)
  using GE = RollGeo<NTO, NHT, 16 * RT>;
  constexpr int H = 256, LDX = GE::LDX, LDH = GE::LDH, LDP = GE::LDP, NHP = GE::NHP, R = 16 * RT;
  float* XS = lds + GE::oXS;
  float* HB = lds + GE::oHB;
  float* SP = lds + GE::oSP;
  float* HBIAS = lds + GE::oHBIAS;
  float* RED = lds + GE::oRED;
  float* HP = lds + GE::oHP;
  float* PRE = lds + GE::oPRE;
  const int lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  f4 acc[2][RT];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const f4 b1 = *reinterpret_cast<const f4*>(SP + GE::sB1 + 32 * wave + 16 * u + 4 * g);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[u][rt] = b1;
  }
  const float* xin = XS + j * LDX + 4 * g;
  act_layer_regs<NTO, RT>(acc, w1, [&](int t, int rt) { return *reinterpret_cast<const f4*>(xin + 16 * rt * LDX + 16 * t); });
#ifdef RDBG
  const bool dbg = stamp_t == 0 && RT == 1 && (int)blockIdx.x * 16 + j == kRdbgEnv;
  auto dump = [&](int base) {
    if (dbg)
      for (int u = 0; u < 2; ++u)
        for (int r = 0; r < 4; ++r) RDBG(0, base + 32 * wave + 16 * u + 4 * g + r, acc[u][0][r]);
  };
#else
  auto dump = [](int) {};
#endif
  dump(0);
  act_activate<PPO_NET_LN_BETA, RT>(acc, SP + GE::sG1, SP + GE::sBE1, RED, wave, j, g);
  dump(260);
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
      *reinterpret_cast<f4*>(HB + (16 * rt + j) * LDH + 32 * wave + 16 * u + 4 * g) = acc[u][rt];
  lds_barrier();
  if (stamp_t >= 0) ROLL_STAMP(stamp_t, 5);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const f4 b2 = *reinterpret_cast<const f4*>(SP + GE::sB2 + 32 * wave + 16 * u + 4 * g);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[u][rt] = b2;
  }
  const float* hin = HB + j * LDH + 4 * g;
  // independent VALU work placed in the layer-2 block: the scheduler interleaves it with the MFMAs,
  // whose issue leaves the SIMD's vector pipe mostly free
  if constexpr (!std::is_same_v<PRE_L2, int>) pre_l2();
  act_layer_regs<16, RT>(acc, w2, [&](int t, int rt) { return *reinterpret_cast<const f4*>(hin + 16 * rt * LDH + 16 * t); });
  if (stamp_t >= 0) {
#ifdef PPO_STAMPS
    asm volatile("s_nop 0" ::"v"(acc[0][0].x), "v"(acc[1][0].x));  // the layer-2 results exist here
#endif
    ROLL_STAMP(stamp_t, 6);
  }
  dump(516);
  act_activate<PPO_NET_LN_BETA, RT>(acc, SP + GE::sG2, SP + GE::sBE2, RED, wave, j, g);
  dump(776);
  if (stamp_t >= 0) ROLL_STAMP(stamp_t, 7);
#pragma unroll
  for (int ht = 0; ht < NHT; ++ht) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      f4 hp = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const f4 wv = *reinterpret_cast<const f4*>(SP + GE::sW3 + (16 * ht + j) * H + 32 * wave + 16 * u + 4 * g);
        hp = mfma16(wv.x, acc[u][rt].x, hp);
        hp = mfma16(wv.y, acc[u][rt].y, hp);
        hp = mfma16(wv.z, acc[u][rt].z, hp);
        hp = mfma16(wv.w, acc[u][rt].w, hp);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) HP[(wave * NHP + 16 * ht + 4 * g + r) * R + 16 * rt + j] = hp[r];
#ifdef RDBG
      if (dbg && ht == 0)
        for (int r = 0; r < 4; ++r) RDBG(0, 1032 + wave * 16 + 4 * g + r, hp[r]);
#endif
    }
  }
  lds_barrier();
  if constexpr (!PRE_PASS) return;
  for (int idx = tid; idx < R * nh; idx += kActThreads) {
    const int r = idx / nh, h = idx - r * nh;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < kActWaves; ++w) s += HP[(w * NHP + h) * R + r];
    PRE[r * LDP + h] = s + HBIAS[h];
  }
  lds_barrier();
}

// this wave's register slices of a trunk's W1 (NTO k-blocks) and W2 (16 k-blocks), 2 feature tiles
template <int NTO>
PPO_DEV void load_weight_slices(PBuf wsw, int wave, int lane, f4 (&w1)[NTO][2], f4 (&w2)[16][2]) {
  constexpr int H = 256, OP = NTO * 16;
  const int l1 = ((2 * wave) * NTO * 64 + lane) * 4;
  const int l2 = H * OP + ((2 * wave) * 16 * 64 + lane) * 4;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
#pragma unroll
    for (int t = 0; t < NTO; ++t) w1[t][u] = pld4(wsw, l1, 256 * (NTO * u + t));
#pragma unroll
    for (int t = 0; t < 16; ++t) w2[t][u] = pld4(wsw, l2, 256 * (16 * u + t));
  }
}

}  // namespace
