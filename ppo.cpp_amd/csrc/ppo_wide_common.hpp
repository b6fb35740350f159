// ppo_wide_common.hpp — what the persistent kernels of the AC agent at Humanoid width share: k_eval_w
// (ppo_eval_wide.hip), k_rollout_w (ppo_rollout_wide.hip) and k_values_w (ppo_values_wide.hip). The LDS
// carve of the first two with one region for XS, HB, HP and ITM in turn (WideGeo), and layer 1 with W1
// streamed from L2 through a ring of k-blocks (ring_fill, layer1_ring). DESIGN 3d, "k_eval_w".
#pragma once

#include "ppo_rollout_common.hpp"

namespace {

constexpr int kRing = 8;  // k-blocks of W1 in flight per wave (2 tiles each: 64 VGPRs)

template <int NTO, int NHT>
struct WideGeo {
  static constexpr int H = 256, OP = NTO * 16, NHP = 16 * NHT, R = kRows;
  static constexpr int LDX = ((OP + 63) / 64) * 64 + 4;
  static constexpr int LDH = H + 4;
  static constexpr int LDP = NHP + 4;
  static constexpr int LDQ = OP + 1;  // env state / obs rows (O <= OP)
  static constexpr int NSP = 6 * H + NHP * H;
  static constexpr int cmax(int a, int b) { return a > b ? a : b; }
  // XS -> HB -> HP -> ITM in turn, a barrier between any two
  static constexpr int nXS = R * LDX, nHB = R * LDH, nHP = kActWaves * NHP * R, nITM = R * 24 * 2 * 4;
  static constexpr int nU = cmax(cmax(nXS, nHB), cmax(nHP, nITM));
  static constexpr int oU = 0;
  static constexpr int oSP = oU + nU;           // b1 g1 be1 b2 g2 be2, the NHP head rows
  static constexpr int oHBIAS = oSP + NSP;
  static constexpr int oRED = oHBIAS + NHP;     // LayerNorm row sums, 2 x 8 x 16
  static constexpr int oPRE = oRED + 2 * kActWaves * R;
  static constexpr int oXO = oPRE + R * LDP;    // agent input obs of the current step
  static constexpr int oQ = oXO + R * LDQ;      // env state q
  static constexpr int oNRM = oQ + R * LDQ;     // obs mean | std (OP each)
  static constexpr int oACT = oNRM + 2 * OP;    // actions [16][24]
  static constexpr int oENV = oACT + R * 24;    // per-env scalars, 16 x 16
  static constexpr int total = oENV + 16 * R;
  static constexpr int sB1 = 0, sG1 = H, sBE1 = 2 * H, sB2 = 3 * H, sG2 = 4 * H, sBE2 = 5 * H, sW3 = 6 * H;
  static_assert(oSP % 4 == 0 && LDX % 4 == 0 && LDH % 4 == 0, "f4 accesses of XS / HB / SP");
  static_assert(total * sizeof(float) <= 160 * 1024, "WideGeo: the LDS carve exceeds a CU's 160 KB");
};

// Layer 1 for this wave's 2 output tiles of the 16 RT rows in XS (row tile rt starts LDT floats after
// row tile rt - 1; RT = 1: k_eval_w / k_rollout_w, RT = 2: k_values_w), the A operands streamed through
// the ring w, whose slot p the caller has filled with k-block p (ring_fill, issued before the rows are
// normalised). One ring load of a k-block feeds the MFMAs of all RT row tiles. This is
// act_layer<NKB, D, RT> (ppo_act_common.hpp) said a second time for two things it does not do: the
// ring's first fill is the caller's, one phase earlier, and the next k-block's B operands are read from
// LDS under this k-block's MFMAs instead of in front of their own. Each accumulator sees k-blocks
// 0 .. NKB - 1 ascending and .x .y .z .w within a block, as in act_layer / act_layer_regs, so the
// results are bitwise theirs.
template <int NKB, int D>
PPO_DEV void ring_fill(f4 (&w)[D][2], PBuf wb, int wlane) {
#pragma unroll
  for (int p = 0; p < D; ++p)
#pragma unroll
    for (int u = 0; u < 2; ++u) w[p][u] = pld4(wb, wlane, 256 * (NKB * u + p));
}
template <int NKB, int D, int LDT = 0, int RT>
PPO_DEV void layer1_ring(f4 (&acc)[2][RT], f4 (&w)[D][2], PBuf wb, int wlane, const float* xin) {
  static_assert(D <= NKB, "ring deeper than the layer");
  static_assert(RT == 1 || LDT > 0, "more than one row tile needs the tiles' stride");
  f4 b[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) b[rt] = *reinterpret_cast<const f4*>(xin + LDT * rt);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < NKB; ++t) {
    f4 bn[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) bn[rt] = *reinterpret_cast<const f4*>(xin + LDT * rt + 16 * (t + 1 < NKB ? t + 1 : t));
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[u][rt] = mfma16(w[t % D][u][c], b[rt][c], acc[u][rt]);
    if (t + D < NKB) {
#pragma unroll
      for (int u = 0; u < 2; ++u) w[t % D][u] = pld4(wb, wlane, 256 * (NKB * u + t + D));
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) b[rt] = bn[rt];
    // keeps the refill where it is written (the scheduler otherwise sinks it towards its use)
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace
