// ppo_eval_wide.hip — k_eval_w: the persistent policy evaluation kernel of the AC agent (LayerNorm-Beta,
// H = 256) at Humanoid width: OP = 384 (O <= 384), 33 <= 2 A <= 48, the cheetah-shaped device env
// without a wrapper chain (ppo_evaluate_synth; ac:965-1001). k_eval (ppo_eval.hip) serves OP <= 32.
//
// k_eval's contract: one launch per chunk of T env steps, one 512-thread workgroup owns 16 envs of
// [0, nE) for the whole chunk, obs -> normalise -> actor -> mean | roach | sample -> clip -> env step ->
// obs with LDS barriers only, the episode events the only global writes of the loop, env_slots_load /
// env_slots_store around it. The actor's chain is k_act3<LN_BETA, 24, 3>'s and the env step
// k_synth_step_wide's, op for op, so every action, observation and return is bitwise the per-step
// path's (tests/test_gpu_eval_wide.py).
//
// k_eval's geometry does not carry over, so this kernel has its own ("k_eval_w"):
//  * registers: a wave's W2 slice stays resident (16 k-blocks x 2 tiles, 128 VGPRs); its W1 slice
//    (24 k-blocks x 2 tiles, 48 KB, contiguous in the MFMA-order copy) does not fit beside it and is
//    streamed every step from L2 through a ring of kRing k-blocks (64 VGPRs). The ring's first fill
//    is issued before the rows are normalised, so its round trip passes under that phase; the ring is
//    dead after layer 1, which leaves the Beta draws and the env step's 12 state chunks per lane their
//    registers (a ring kept filled across the step boundary spills at every depth above 3).
//  * LDS: the input rows (XS), the hidden rows (HB), the head partials (HP) and the Beta items (ITM)
//    are live one after the other, with a workgroup barrier between any two of them, and share one
//    region (WideGeo::oU). With that the carve is 139 584 B; RollGeo<24, 3> needs 180 800 B.
//  * Beta items: 16 A 2 = 544 (A = 17) to 768 (A = 24) items on 512 threads, so a thread loops over
//    item tid, tid + 512. The Philox keys are (seed, rank, env, step, item), as everywhere.
// WideGeo, kRing, ring_fill, layer1_ring (shared with k_rollout_w, ppo_rollout_wide.hip)
#include "ppo_wide_common.hpp"

template <int NTO, int NHT, int KIND = PSYN_CHEETAH>
__global__ __launch_bounds__(512) void k_eval_w(EvalArgs a) {
  static_assert(KIND == PSYN_CHEETAH, "k_eval_w: the cheetah-shaped env (a kind with a DevEnv has O <= 32: k_eval)");
  using GE = WideGeo<NTO, NHT>;
  constexpr int H = GE::H, OP = GE::OP, NHP = GE::NHP, LDX = GE::LDX, LDH = GE::LDH, LDP = GE::LDP, LDQ = GE::LDQ;
  constexpr int R = kRows;
  constexpr int NCH = (OP + 31) / 32;  // 32-dim chunks of the env state per env lane group
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* XS = lds + GE::oU;
  float* HB = lds + GE::oU;
  float* HP = lds + GE::oU;
  float* ITM = lds + GE::oU;
  float* SP = lds + GE::oSP;
  float* HBIAS = lds + GE::oHBIAS;
  float* RED = lds + GE::oRED;
  float* PRE = lds + GE::oPRE;
  float* XO = lds + GE::oXO;
  float* Q = lds + GE::oQ;
  float* NRM = lds + GE::oNRM;
  float* ACT = lds + GE::oACT;
  float* EV = lds + GE::oENV;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const PackedLayout& K = a.K;
  const float* __restrict__ P = a.P;
  const PBuf pb = make_pbuf(P, K.size);
  const int O = K.O, A = K.A, E = a.nE;  // the evaluated envs [0, nE); the env's other envs are not touched
  const int row0 = blockIdx.x * R;
  const SynthArgs& sv = a.env;

  // ---- prologue: W2 resident, staged parameters, env state of this block ----
  const PBuf wsw = make_pbuf(a.WSW, (int)sw_size(H, OP));
  const int l1 = ((2 * wave) * NTO * 64 + lane) * 4;
  f4 w2[16][2];
  {
    const int l2 = H * OP + ((2 * wave) * 16 * 64 + lane) * 4;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int t = 0; t < 16; ++t) w2[t][u] = pld4(wsw, l2, 256 * (16 * u + t));
    }
  }
  stage_params<NHP>(K, K.tr[1], pb, 1, SP, HBIAS, tid);
  for (int f = tid; f < OP; f += kActThreads) {
    NRM[f] = f < O ? P[K.omean + f] : 0.0f;
    NRM[OP + f] = f < O ? P[K.ostd + f] : 1.0f;
  }
  env_slots_load<R, kActThreads>(EV, XO, Q, LDQ, sv, a.obs, nullptr, row0, E, O, tid);
  lds_barrier();
  const SampleKey key = sample_key(a.seed, a.rank);
  const float hi = P[K.hi], lo = P[K.lo];
  const bool sample = a.mode == PPO_SAMPLE;
  const int nitem = R * A * 2;

  for (int t = 0; t < a.T; ++t) {
    const long step_id = a.step0 + t;
    // tid, opaque to the compiler once per step. The index arithmetic of the phases that use it (the 12
    // env dims' i % A, the items' idx / A, the rows' idx / OP) does not depend on the step; hoisted out
    // of this loop it stays in VGPRs across layer 1, where W2 and the ring leave it none (scratch)
    int td = tid;
    asm volatile("" : "+v"(td));
    // W1's first kRing k-blocks: no input of theirs depends on the step, so their L2 round trip passes
    // under the normalisation
    f4 ring[kRing][2];
    ring_fill<NTO, kRing>(ring, wsw, l1);
    // ---- normalised rows into XS (k_act3 order) ----
    for (int idx = td; idx < R * OP; idx += kActThreads) {
      const int r = idx / OP, f = idx - r * OP, e = row0 + r;
      const bool valid = e < E && f < O;
      const float x = valid ? XO[r * LDQ + f] : 0.0f;
      XS[r * LDX + f] = valid ? (x - NRM[f]) / NRM[OP + f] : x;
    }
    lds_barrier();
    // ---- layer 1 (W1 through the ring), LayerNorm + ReLU ----
    f4 acc[2][1];
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[u][0] = *reinterpret_cast<const f4*>(SP + GE::sB1 + 32 * wave + 16 * u + 4 * g);
    layer1_ring<NTO, kRing>(acc, ring, wsw, l1, XS + j * LDX + 4 * g);
    act_activate<PPO_NET_LN_BETA, 1>(acc, SP + GE::sG1, SP + GE::sBE1, RED, wave, j, g);
    // every wave is past act_activate's barriers: XS is dead, HB takes its place
#pragma unroll
    for (int u = 0; u < 2; ++u) *reinterpret_cast<f4*>(HB + j * LDH + 32 * wave + 16 * u + 4 * g) = acc[u][0];
    lds_barrier();
    // ---- layer 2 (W2 resident), LayerNorm + ReLU ----
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[u][0] = *reinterpret_cast<const f4*>(SP + GE::sB2 + 32 * wave + 16 * u + 4 * g);
    // PPO_SAMPLE: the first Marsaglia-Tsang attempt's draws of this thread's first item do not depend
    // on the network; computed under layer 2's MFMAs (gamma_mt_d0 with them is gamma_mt, bitwise)
    GammaDraw gd0 = GammaDraw{0.f, 0.f};
    if (sample && td < nitem) {
      const BetaItem bi = beta_item(td, A);
      gd0 = gamma_draw(key, (long)(row0 + bi.r), step_id, bi.db);
    }
    const float* hin = HB + j * LDH + 4 * g;
    act_layer_regs<16, 1>(acc, w2, [&](int kb, int) { return *reinterpret_cast<const f4*>(hin + 16 * kb); });
    act_activate<PPO_NET_LN_BETA, 1>(acc, SP + GE::sG2, SP + GE::sBE2, RED, wave, j, g);
    // ---- heads: split-K partials over this wave's 32 features, NHT tiles; HB is dead, HP takes its place ----
#pragma unroll
    for (int ht = 0; ht < NHT; ++ht) {
      f4 hp = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const f4 wv = *reinterpret_cast<const f4*>(SP + GE::sW3 + (16 * ht + j) * H + 32 * wave + 16 * u + 4 * g);
        hp = mfma16(wv.x, acc[u][0].x, hp);
        hp = mfma16(wv.y, acc[u][0].y, hp);
        hp = mfma16(wv.z, acc[u][0].z, hp);
        hp = mfma16(wv.w, acc[u][0].w, hp);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) HP[(wave * NHP + 16 * ht + 4 * g + r) * R + j] = hp[r];
    }
    lds_barrier();
    // waves 0 .. 7 ascending, then + HBIAS: k_act3's (and trunk_rows') order
    for (int idx = td; idx < R * 2 * A; idx += kActThreads) {
      const int r = idx / (2 * A), h = idx - r * (2 * A);
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < kActWaves; ++w) s += HP[(w * NHP + h) * R + r];
      PRE[r * LDP + h] = s + HBIAS[h];
    }
    lds_barrier();
    // ---- concentrations (k_act3 stage 1) and the action on [0, 1] (stage 2); HP is dead, ITM takes its place ----
    for (int idx = td; idx < nitem; idx += kActThreads) {
      const BetaItem bi = beta_item(idx, A);
      const long env = row0 + bi.r;
      const float c = softplusf_(PRE[bi.r * LDP + bi.ai + bi.which * A]) + 1.0f;
      float gs = 0.f;
      if (sample) gs = idx == td ? gamma_mt_d0(c, gd0, key, env, step_id, bi.db) : gamma_mt(c, key, env, step_id, bi.db);
      float* it = ITM + idx * 4;  // ((r A + ai) 2 + which) 4
      it[0] = c;
      it[1] = gs;
    }
    lds_barrier();
    for (int idx = td; idx < R * A; idx += kActThreads) {
      const int r = idx / A, ai = idx - r * A;
      const float* ia = ITM + (idx * 2 + 0) * 4;
      const float* ib = ITM + (idx * 2 + 1) * 4;
      const float al = ia[0], be = ib[0];
      float s01;  // k_eval's three-way switch
      if (a.mode == PPO_MEAN) s01 = al / (al + be);
      else if (a.mode == PPO_ROACH) s01 = beta_roach01(al, be);
      else s01 = beta_sample01(ia[1], ib[1]);
      ACT[r * 24 + ai] = beta_action(s01, lo, hi);
    }
    lds_barrier();
    // ---- env step: 32 lanes per env, NCH dims each (k_synth_step_wide's arithmetic); an episode that
    // is truncated is one event ----
    {
      const int r = td >> 5, i0 = td & 31, e = row0 + r;
      if (e < E) {
        chee_lanes_step<R, NCH>(EV, r, i0, O, A, Q + r * LDQ, XO + r * LDQ, ACT + r * 24, a.lo, a.hi,
                                [&](const EnvLaneOut& o) {
                                  if (o.fin) {
                                    const unsigned slot = atomicAdd(a.count, 1u);
                                    if (slot < (unsigned)a.cap) a.ev[slot] = EvalEvent{a.k0 + t, e, o.epl, o.epr};
                                  }
                                });
      }
    }
    lds_barrier();
  }
  // ---- epilogue: the obs and the env state back to HBM (the next chunk continues from them) ----
  env_slots_store<R, kActThreads>(EV, XO, Q, LDQ, sv, a.obs, nullptr, row0, E, O, tid);
}

// 0 when k_eval_w covers the agent (AC agent, H = 256, OP = 384, three head tiles: 17 <= A <= 24)
int eval_w_supported(const PackedLayout& K) {
  return (K.kind == PPO_NET_LN_BETA && K.H == 256 && K.OP == 384 && 2 * K.A >= 33 && 2 * K.A <= 48) ? 0 : -1;
}

int launch_eval_w(const EvalArgs& a, hipStream_t s) {
  if (eval_w_supported(a.K) != 0 || a.env.w.on || a.env.kind != PSYN_CHEETAH || a.nE <= 0 || a.T <= 0) return -1;
  if (a.mode != PPO_SAMPLE && a.mode != PPO_MEAN && a.mode != PPO_ROACH) return -1;
  using GE = WideGeo<24, 3>;
  const size_t lds = (size_t)GE::total * sizeof(float);
  static const bool ok = hipFuncSetAttribute((const void*)k_eval_w<24, 3, PSYN_CHEETAH>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
  if (!ok) return -2;
  hipLaunchKernelGGL((k_eval_w<24, 3, PSYN_CHEETAH>), dim3((a.nE + kRows - 1) / kRows), dim3(kActThreads), lds, s, a);
  return 0;
}
