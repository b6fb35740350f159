// ppo_rollout_split.hip — k_rollout_s: the AC agent's persistent rollout for few envs per GPU with
// the layers' k range split over wave halves (create option rollout_kernel=split; DESIGN §3b').
//
// k_rollout_v (ppo_rollout.hip) is tied bit for bit to the MFMA rollout: every output feature is one
// serial 256-long FMA chain in the MFMA's k order, half of W2 is re-read from LDS every step, and it
// steps the synthetic cheetah only. k_rollout_s keeps the loop contract (2 envs per workgroup, one
// launch for all T steps, the same rollout stores, Philox keys, Beta sampling and env step) and lets
// the trunk reassociate; it is judged against the fp64 oracle, not against k_rollout's bits:
//  * 8 waves = 4 feature quarters x 2 k-halves. A lane owns output feature f = 64 (wave & 3) + lane
//    for BOTH envs of the workgroup and keeps W2[f][128 kh .. 128 kh + 127] (kh = wave >> 2) in
//    registers for the rollout: W2 has no LDS copy and no per-step read. W1 (at most 32 KB) lies in
//    LDS, lane-consecutive float4s (in registers next to the 128 resident weights it spilled);
//  * layer 2: 128 k's x 2 rows per lane as 4 independent accumulators (2 rows x even / odd k), so a
//    dependent FMA is 4 issues away; the k-halves' partial sums meet in LDS and are added in the
//    fixed order (half 0 + half 1) by every wave, so results do not depend on timing;
//  * layer 1 (OP <= 32 k's) is computed whole by both k-halves: no exchange, the same bits twice;
//  * layer inputs: lane k of every 16-lane row holds the inputs 16 i + k of both rows (loaded with
//    two / four ds_read_b128 from a k-major LDS layout) and v_fmac_f32_dpp row_newbcast:k hands
//    input k to the row's 16 lanes: no broadcast LDS read per k (4 LDS cycles each, §3b);
//  * LayerNorm: wave sums by DPP / permlane swaps, one LDS exchange across the 4 feature waves, both
//    rows at once; mean first, then the squares of the deviations;
//  * heads, Beta sample, env step (env_lanes_step<KIND, 2, NCH>: every device env kind) and the next
//    step's first gamma draws under the env step are k_rollout_v's.
// This file is compiled with packed fp32 instructions off (Makefile: a choice, it has no spills either
// way). The two rows of a lane are therefore two v_fmac_f32_dpp, not one v_pk_fma_f32: the DPP
// broadcast has no packed form (DESIGN §3b').
#include "ppo_act_common.hpp"

#include <type_traits>

using namespace act;

#ifdef PPO_STAMPS
// diagnostic build only: shader-clock stamps at the 9 phase ends of the first 16 steps, wave 0 of
// workgroup 0; read with ppo_diag_read_roll_s_stamps
__device__ unsigned long long g_roll_s_stamps[16 * 16];
#define ROLL_STAMP(t, k)                                                                      \
  do {                                                                                        \
    if (blockIdx.x == 0 && threadIdx.x == 0 && (t) < 16)                                      \
      g_roll_s_stamps[(t) * 16 + (k)] = __builtin_amdgcn_s_memtime();                        \
  } while (0)
extern "C" int ppo_diag_read_roll_s_stamps(unsigned long long* host, long n) {
  if (n > 16 * 16) n = 16 * 16;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_roll_s_stamps), n * sizeof(unsigned long long), 0,
                             hipMemcpyDeviceToHost) == hipSuccess ? (int)n : -2;
}
#endif

#include "ppo_rollout_common.hpp"

namespace {
template <int NTO>
struct RollSGeo {
  static constexpr int R = 2, H = 256, OP = NTO * 16, NHP = 16, LDZ = H + 4, LDQ = OP + 1;
  // layer inputs, k-major: input 16 i + k of row r at [k][r][i], so lane k of every 16-lane row loads
  // its inputs of both rows as one contiguous run. Layer 1: [16][R][2] (i < NTO <= 2). Layer 2, per
  // k-half: [16][LDK], R x 8 inputs and 4 floats of padding (stride 20: conflict-free ds_read_b128)
  static constexpr int LDK = 20;
  static constexpr int oXV = 0;
  static constexpr int oHV = oXV + 16 * R * 2;      // [2 k-halves][16][LDK]
  static constexpr int oZP = oHV + 2 * 16 * LDK;    // layer-2 partial sums [2 k-halves][R][H]
  static constexpr int oH2 = oZP + 2 * R * H;       // head inputs h2 [R][LDZ]
  static constexpr int oRS = oH2 + R * LDZ;         // LayerNorm exchange [2 k-halves][sums | squares][4 quarters][R]
  static constexpr int oW3 = oRS + 2 * 2 * 4 * R;   // head rows [NHP][H]
  static constexpr int oHB = oW3 + NHP * H;         // head biases [NHP]
  static constexpr int oHP = oHB + NHP;             // head partials [8][NHP][R]
  static constexpr int oXO = oHP + 8 * NHP * R;     // agent input obs of the step [R][LDQ]
  static constexpr int oQ = oXO + R * LDQ;          // env state q [R][LDQ]
  static constexpr int oNRM = oQ + R * LDQ;         // obs mean | std [2][OP]
  static constexpr int oACT = oNRM + 2 * OP;        // actions [R][24]
  static constexpr int oENV = oACT + R * 24;        // per-env scalars [16][R]
  static constexpr int oW1 = oENV + 16 * R;         // W1 [OP / 4][H] float4s: inputs 4 q .. 4 q + 3 of feature f at [q][f]
  static constexpr int total = oW1 + OP * H;
  static_assert(oHV % 4 == 0 && oZP % 4 == 0 && oH2 % 4 == 0 && oRS % 4 == 0 && oW3 % 4 == 0, "float4 regions");
  static_assert(oW1 % 4 == 0, "float4 region");
  static_assert(total * sizeof(float) <= 64 * 1024, "k_rollout_s LDS above the default 64 KB");
};

// (a0, a1) += w * (x0, x1) taken from lane K of this lane's 16-lane row: the two rows' FMAs of one
// weight, back to back. x0 / x1 come from LDS loads and an s_nop 1 precedes each chain, so no VALU
// instruction writes a DPP source within the two wait states before it (tests/test_isa_dpp_hazard.py
// states the rule; tests/test_isa_rollout_split.py checks this file's object).
template <int K>
PPO_DEV void fmac2_bc(float& a0, float& a1, float x0, float x1, float w) {
  asm volatile("v_fmac_f32_dpp %0, %2, %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
               "v_fmac_f32_dpp %1, %3, %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf"
               : "+v"(a0), "+v"(a1)
               : "v"(x0), "v"(x1), "v"(w), "n"(K));
}
// the sum over the wave's 64 lanes, the same bits in every lane
PPO_DEV float wave_sum(float v) {
  v = group8_sum(v);
  v += dpp_f<kDppRowRor8>(v);
  return xor32_sum(xor16_sum(v));
}
}  // namespace

constexpr int kRSThreads = 512;
template <int NTO, int KIND>
__global__ __launch_bounds__(kRSThreads) void k_rollout_s(RolloutArgs a) {
  static_assert(psyn_kind_tiles_ok<KIND, NTO, 1>(), PSYN_KIND_TILES_MSG);
  using GE = RollSGeo<NTO>;
  constexpr int R = GE::R, H = 256, OP = GE::OP, NHP = GE::NHP, LDZ = GE::LDZ, LDQ = GE::LDQ, LDK = GE::LDK;
  constexpr int NCH = (OP + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* XV = lds + GE::oXV;
  float* HV = lds + GE::oHV;
  float* ZP = lds + GE::oZP;
  float* H2 = lds + GE::oH2;
  float* W3 = lds + GE::oW3;
  float* HBIAS = lds + GE::oHB;
  float* HP = lds + GE::oHP;
  float* XO = lds + GE::oXO;
  float* Q = lds + GE::oQ;
  float* NRM = lds + GE::oNRM;
  float* ACT = lds + GE::oACT;
  float* EV = lds + GE::oENV;
  float* W1L = lds + GE::oW1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fq = wave & 3, kh = wave >> 2, f = 64 * fq + lane;  // feature quarter, k-half, output feature
  float* RS = lds + GE::oRS + kh * 16;                          // this k-half's exchange: sums [4][R], squares [4][R]
  const PackedLayout& K = a.K;
  const TrunkDev& T = K.tr[1];
  const float* __restrict__ P = a.P;
  const int O = K.O, A = K.A, E = a.E, nh = 2 * A;
  const int row0 = blockIdx.x * R;
  const SynthArgs& sv = a.env;

  // ---- prologue: this lane's k-half of its W2 row, W1 and the head rows staged, env state ----
  float w2r[128];
  for (int i = tid; i < OP / 4 * H; i += kRSThreads) {
    const int q = i / H, ff = i - q * H;
    st4(W1L + 4 * i, ld4(P + T.W1 + (long)ff * OP + 4 * q));
  }
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const f4 v = ld4(P + T.W2 + (long)f * H + 128 * kh + 4 * i);
#pragma unroll
    for (int c = 0; c < 4; ++c) w2r[4 * i + c] = v[c];
  }
  const float b1 = P[T.b1 + f], b2 = kh == 0 ? P[T.b2 + f] : 0.0f;  // the layer-2 bias enters in k-half 0
  const float g1 = P[T.g1 + f], be1 = P[T.be1 + f], g2 = P[T.g2 + f], be2 = P[T.be2 + f];
  for (int i = tid; i < NHP * H; i += kRSThreads) {
    const int h = i / H, k = i - h * H;
    const int hr = act_head_row(K, 1, h);
    W3[i] = hr >= 0 ? P[hr + k] : 0.0f;
  }
  if (tid < NHP) {
    const int hbo = act_head_bias(K, 1, tid);
    HBIAS[tid] = hbo >= 0 ? P[hbo] : 0.0f;
  }
  for (int i = tid; i < OP; i += kRSThreads) {
    NRM[i] = i < O ? P[K.omean + i] : 0.0f;
    NRM[OP + i] = i < O ? P[K.ostd + i] : 1.0f;
  }
  if (tid < 16 * R * 2) XV[tid] = 0.0f;  // NTO = 1 never writes the i = 1 slots
  env_slots_load<R, kRSThreads>(EV, XO, Q, LDQ, sv, a.next_obs, a.next_done, row0, E, O, tid);
  lds_barrier();
  const SampleKey key = sample_key(a.seed, a.rank);
  const float hi = P[K.hi], lo = P[K.lo];
  // Beta items (row, action, alpha | beta) spread evenly over waves 1-7, which are idle during the
  // env step (wave 0): the next step's first Marsaglia-Tsang draws are computed there. An even
  // count per wave keeps an action's alpha and beta items in adjacent lanes (2 m, 2 m + 1)
  const int bper = 2 * ((R * A + 6) / 7);
  const int bitem = (wave > 0 && lane < bper) ? (wave - 1) * bper + lane : R * A * 2;
  auto draw0 = [&](long step) {
    GammaDraw d = GammaDraw{0.f, 0.f};
    if (bitem < R * A * 2) {
      const BetaItem bi = beta_item(bitem, A);
      d = gamma_draw(key, (long)(row0 + bi.r), step, bi.db);
    }
    return d;
  };
  GammaDraw gd0 = draw0(a.step0);
  // LayerNorm + ReLU of this lane's feature of both rows (z0, z1 in, activations out): the wave's
  // sums meet the other 3 feature quarters' in RS, added in quarter order; 2 barriers. RS is not
  // rewritten before other barriers, so none follows the last read.
  auto ln_relu = [&](float& z0, float& z1, float gm, float bt) {
    const float s0 = wave_sum(z0), s1 = wave_sum(z1);
    if (lane == 0) {
      RS[fq * R + 0] = s0;
      RS[fq * R + 1] = s1;
    }
    lds_barrier();
    const f4 sa = ld4(RS), sb = ld4(RS + 4);  // (quarter 0: row 0, row 1; quarter 1: ...), (quarters 2, 3)
    const float mu0 = ((sa.x + sa.z) + (sb.x + sb.z)) * (1.0f / 256);
    const float mu1 = ((sa.y + sa.w) + (sb.y + sb.w)) * (1.0f / 256);
    const float d0 = z0 - mu0, d1 = z1 - mu1;
    const float q0 = wave_sum(__fmul_rn(d0, d0)), q1 = wave_sum(__fmul_rn(d1, d1));
    if (lane == 0) {
      RS[8 + fq * R + 0] = q0;
      RS[8 + fq * R + 1] = q1;
    }
    lds_barrier();
    const f4 qa = ld4(RS + 8), qb = ld4(RS + 12);
    const float rs0 = 1.0f / sqrtf(__fmaf_rn((qa.x + qa.z) + (qb.x + qb.z), 1.0f / 256, 1e-5f));
    const float rs1 = 1.0f / sqrtf(__fmaf_rn((qa.y + qa.w) + (qb.y + qb.w), 1.0f / 256, 1e-5f));
    const float y0 = __fmaf_rn(gm, __fmul_rn(d0, rs0), bt), y1 = __fmaf_rn(gm, __fmul_rn(d1, rs1), bt);
    z0 = y0 > 0.0f ? y0 : 0.0f;
    z1 = y1 > 0.0f ? y1 : 0.0f;
  };
  const int kl = lane & 15;  // this lane's position in its 16-lane row
  const float* xv = XV + kl * 4;
  const float* hv = HV + (kh * 16 + kl) * LDK;
  // where this lane's layer-1 activation goes as a layer-2 input: k = f, k-half f >> 7
  float* hst = HV + ((f >> 7) * 16 + (f & 15)) * LDK + ((f & 127) >> 4);

  for (int t = 0; t < a.T; ++t) {
    const long step_id = a.step0 + t;
    ROLL_STAMP(t, 0);
    // ---- inputs: rollout stores of obs[t] / dones[t]; normalised rows into XV ----
    for (int idx = tid; idx < R * OP; idx += kRSThreads) {
      const int r = idx / OP, ff = idx - r * OP, e = row0 + r;
      const bool valid = e < E && ff < O;
      const float x = valid ? XO[r * LDQ + ff] : 0.0f;
      if (valid) a.s_obs[((long)t * E + e) * O + ff] = x;
      XV[(ff & 15) * 4 + r * 2 + (ff >> 4)] = valid ? (x - NRM[ff]) / NRM[OP + ff] : x;
    }
    if (tid < R && row0 + tid < E) a.s_dones[(long)t * E + row0 + tid] = EV[EV_DONE * R + tid];
    lds_barrier();
    ROLL_STAMP(t, 1);
    // ---- layer 1, whole in every wave: rows 0 / 1, even / odd k ----
    float z0 = b1, z1 = b1;
    {
      float y0 = 0.0f, y1 = 0.0f;
      const f4 x = ld4(xv);  // (row 0: inputs kl, 16 + kl; row 1: the same)
      f4 w1q[OP / 4];
#pragma unroll
      for (int q = 0; q < OP / 4; ++q) w1q[q] = ld4(W1L + (q * H + f) * 4);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 1" ::: "memory");
      static_for<OP>([&](auto P_) {
        constexpr int p = decltype(P_)::value;
        if constexpr (p & 1) fmac2_bc<p & 15>(y0, y1, x[p >> 4], x[2 + (p >> 4)], w1q[p >> 2][p & 3]);
        else fmac2_bc<p & 15>(z0, z1, x[p >> 4], x[2 + (p >> 4)], w1q[p >> 2][p & 3]);
      });
      z0 += y0;
      z1 += y1;
    }
    ROLL_STAMP(t, 2);
    ln_relu(z0, z1, g1, be1);
    hst[kh * 8] = kh ? z1 : z0;  // k-half kh's waves store row kh (both halves hold both rows)
    lds_barrier();
    ROLL_STAMP(t, 3);
    // ---- layer 2, this wave's k-half: the inputs 16 i + kl of both rows, 8 + 8 per lane ----
    z0 = b2;
    z1 = b2;
    {
      float y0 = 0.0f, y1 = 0.0f;
      float x0[8], x1[8];
      *reinterpret_cast<f4*>(x0) = ld4(hv);
      *reinterpret_cast<f4*>(x0 + 4) = ld4(hv + 4);
      *reinterpret_cast<f4*>(x1) = ld4(hv + 8);
      *reinterpret_cast<f4*>(x1 + 4) = ld4(hv + 12);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 1" ::: "memory");
      static_for<128>([&](auto P_) {
        constexpr int p = decltype(P_)::value;
        if constexpr (p & 1) fmac2_bc<p & 15>(y0, y1, x0[p >> 4], x1[p >> 4], w2r[p]);
        else fmac2_bc<p & 15>(z0, z1, x0[p >> 4], x1[p >> 4], w2r[p]);
      });
      z0 += y0;
      z1 += y1;
    }
    ZP[(kh * R + 0) * H + f] = z0;
    ZP[(kh * R + 1) * H + f] = z1;
    lds_barrier();
    z0 = ZP[f] + ZP[R * H + f];  // k-half 0 + k-half 1, in every wave
    z1 = ZP[H + f] + ZP[(R + 1) * H + f];
    ROLL_STAMP(t, 4);
    ln_relu(z0, z1, g2, be2);
    H2[kh * LDZ + f] = kh ? z1 : z0;
    lds_barrier();
    ROLL_STAMP(t, 5);
    // ---- heads: (head, 32-feature segment, row) partials from float4 reads ----
    for (int idx = tid; idx < nh * 8 * R; idx += kRSThreads) {
      const int r = idx % R, sg = (idx / R) & 7, h = idx / (8 * R);
      float hp0 = 0.f, hp1 = 0.f;
#pragma unroll 1  // unrolled, the 16 float4 operands in flight are the kernel's register peak: every instantiation spills
      for (int u = 0; u < 8; u += 2) {
        const f4 wa = ld4(W3 + h * H + 32 * sg + 4 * u), wb = ld4(W3 + h * H + 32 * sg + 4 * u + 4);
        const f4 xa = ld4(H2 + r * LDZ + 32 * sg + 4 * u), xb = ld4(H2 + r * LDZ + 32 * sg + 4 * u + 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          hp0 = __builtin_fmaf(wa[c], xa[c], hp0);
          hp1 = __builtin_fmaf(wb[c], xb[c], hp1);
        }
      }
      HP[(sg * NHP + h) * R + r] = hp0 + hp1;
    }
    lds_barrier();
    ROLL_STAMP(t, 6);
    // ---- Beta sample (k_rollout_v's): the alpha and beta items of an action sit in adjacent lanes,
    // so the partner's concentration and gamma sample come by DPP (quad xor 1) ----
    float bc = 1.0f, bg = 1.0f;
    if (bitem < R * A * 2) {
      const BetaItem bi = beta_item(bitem, A);
      const int r = bi.r, h = bi.ai + bi.which * A;
      float sm = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) sm += HP[(w * NHP + h) * R + r];
      bc = softplusf_(sm + HBIAS[h]) + 1.0f;
      bg = gamma_mt_d0(bc, gd0, key, (long)(row0 + r), step_id, bi.db);
    }
    {
      const float pc = dpp_f<kDppQuadXor1>(bc), pg = dpp_f<kDppQuadXor1>(bg);  // every lane of the wave
      if (bitem < R * A * 2 && (bitem & 1) == 0) {
        const int ra = bitem >> 1, r = ra / A, ai = ra - r * A, e = row0 + r;
        const float al = bc, be = pc;
        const float s01 = beta_sample01(bg, pg);
        const float act = beta_action(s01, lo, hi);
        ACT[r * 24 + ai] = act;
        if (e < E) {
          a.s_actions[((long)t * E + e) * A + ai] = act;
          float* d = a.s_beta + (((long)t * E + e) * A + ai) * 3;
          d[0] = al;
          d[1] = be;
          d[2] = s01;
        }
      }
    }
    lds_barrier();
    ROLL_STAMP(t, 7);
    // ---- env step: 32 lanes per env, any device env kind ----
    if (tid < 32 * R) {
      const int r = tid >> 5, i0 = tid & 31, e = row0 + r;
      if (e < E) {
        env_lanes_step<KIND, R, NCH>(EV, r, i0, O, A, Q + r * LDQ, XO + r * LDQ, ACT + r * 24, a.lo, a.hi,
                                     [&](const EnvLaneOut& o) {
                                       a.s_rewards[(long)t * E + e] = o.reward;
                                       EV[EV_DONE * R + r] = o.fin ? 1.0f : 0.0f;
                                     });
      }
    }
    // the first Marsaglia-Tsang attempt's draws of the next step (independent of the network)
    if (wave > 0 && t + 1 < a.T) gd0 = draw0(step_id + 1);
    lds_barrier();
    ROLL_STAMP(t, 8);
  }
  // ---- epilogue: next_obs / next_done and the env state back to HBM ----
  env_slots_store<R, kRSThreads>(EV, XO, Q, LDQ, sv, a.next_obs, a.next_done, row0, E, O, tid);
}

template <int NTO, int KIND>
static int launch_rollout_s_t(const RolloutArgs& a, hipStream_t s) {
  const size_t lds = (size_t)RollSGeo<NTO>::total * sizeof(float);
  hipLaunchKernelGGL((k_rollout_s<NTO, KIND>), dim3((a.E + 1) / 2), dim3(kRSThreads), lds, s, a);
  return 0;
}

// rollout_kernel=split (RolloutArgs::variant 3): -5 where the agent or the env cannot take it, -1
// where the env kind's shape is not the agent's
int launch_rollout_s(const RolloutArgs& a, hipStream_t s) {
  if (a.K.kind != PPO_NET_LN_BETA || a.K.H != 256 || a.K.OP > 32 || 2 * a.K.A > 16 || a.env.w.on || !a.s_beta) return -5;
  if (a.env.kind != PSYN_CHEETAH)
    return dispatch_env_kind(a.env.kind, [&](auto KIND_) {
      constexpr int KIND = decltype(KIND_)::value;
      using D = DevEnv<KIND>;
      if (a.K.OP != 16 * D::NTO || a.K.A != D::A) return -1;
      return launch_rollout_s_t<D::NTO, KIND>(a, s);
    });
  return a.K.OP == 16 ? launch_rollout_s_t<1, PSYN_CHEETAH>(a, s) : launch_rollout_s_t<2, PSYN_CHEETAH>(a, s);
}
