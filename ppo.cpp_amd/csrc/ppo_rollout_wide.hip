// ppo_rollout_wide.hip — k_rollout_w: the persistent rollout kernel of the AC agent (LayerNorm-Beta,
// H = 256) at Humanoid width: OP = 384 (O <= 384), 33 <= 2 A <= 48, the cheetah-shaped device env
// without a wrapper chain (ppo_rollout_synth). k_rollout (ppo_rollout.hip) serves OP <= 112, A <= 8.
//
// k_rollout's contract on k_eval_w's geometry (ppo_eval_wide.hip, ppo_wide_common.hpp): one launch for
// all T steps, one 512-thread workgroup owns 16 envs of [0, E) for the whole rollout, obs -> normalise ->
// actor -> Beta sample -> clip -> env step -> obs with LDS barriers only, env_slots_load /
// env_slots_store on next_obs / next_done around the loop. Step t stores obs[t], dones[t], actions[t],
// (alpha, beta, sample)[t] and rewards[t]; the log-probs (k_beta_logp) and the critic run after the
// launch over the stored rows. The actor's chain is k_act3<LN_BETA, 24, 3>'s and the env step
// k_synth_step_wide's, op for op, so every stored value is bitwise the per-step path's
// (tests/test_gpu_rollout_wide.py).
//
// What the stores change ("k_rollout_w"):
//  * registers: k_eval_w leaves 13 VGPRs. A store through a pointer is a 64-bit address per lane and
//    store; here every store goes through a buffer resource of its step's slice of the buffer (a
//    wave-uniform base, built from scalars where it is used) with one 32-bit lane offset. The slice's
//    size is the resource's range: a lane offset past it is dropped by the hardware, not written.
//  * the obs store (16 x O floats per workgroup and step) maps like the env step, 32 lanes per env and
//    12 dims per lane, read back from XO in one batch. It is issued after the ring's first fill and the
//    normalisation, in front of the barrier, which waits for LDS traffic only. Lanes without a dim or an
//    env are masked by an out-of-range offset (kDropped), not by a branch, so the waits on the ring's
//    first fill count the 13 stores behind it and leave them in flight (vmcnt 28 .. 24 where k_eval_w
//    has 15 .. 11); the first refill's data is needed 8 k-blocks (64 MFMAs) after the stores.
//  * the action and (alpha, beta, sample) stores are issued from the action loop (one dword and one
//    three-dword store per action), the reward store from the env step's lane 0; nothing waits on them.
#include "ppo_wide_common.hpp"

namespace {

typedef unsigned int u3 __attribute__((ext_vector_type(3)));

// A lane offset past the range of every slice (launch_rollout_w keeps a buffer below this many bytes):
// the hardware drops the store. The obs and dones stores mask their lanes with it instead of a branch,
// so the stores are straight-line code and the waits on the ring's loads count them exactly (a store
// under a branch makes the compiler wait for the ring as if no store had been issued, which with the
// stores in flight waits for them too).
constexpr unsigned kDropped = 0xFFFFFF00u;

// step t's slice (slice floats long) of a rollout buffer as a buffer resource; wave-uniform
PPO_DEV PBuf step_buf(float* base, int t, unsigned slice) {
  return PBuf{__builtin_amdgcn_make_buffer_rsrc((void*)(base + (size_t)t * slice), (short)0, (int)(slice * 4u), 0x00020000)};
}
// one float / three floats at byte offset lane_bytes of the slice
PPO_DEV void pst1(PBuf b, float v, unsigned lane_bytes) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), b.r, (int)lane_bytes, 0, 0);
}
PPO_DEV void pst3(PBuf b, float x, float y, float z, unsigned lane_bytes) {
  const u3 v = {__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, y), __builtin_bit_cast(unsigned, z)};
  __builtin_amdgcn_raw_buffer_store_b96(v, b.r, (int)lane_bytes, 0, 0);
}

}  // namespace

template <int NTO, int NHT, int KIND = PSYN_CHEETAH>
__global__ __launch_bounds__(512) void k_rollout_w(RolloutArgs a) {
  static_assert(KIND == PSYN_CHEETAH, "k_rollout_w: the cheetah-shaped env (a kind with a DevEnv has O <= 32: k_rollout)");
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
  const int O = K.O, A = K.A, E = a.E;
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
  env_slots_load<R, kActThreads>(EV, XO, Q, LDQ, sv, a.next_obs, a.next_done, row0, E, O, tid);
  lds_barrier();
  const SampleKey key = sample_key(a.seed, a.rank);
  const float hi = P[K.hi], lo = P[K.lo];
  const int nitem = R * A * 2;
  // floats per step of the five stored buffers: obs E O, actions E A, (alpha, beta, sample) 3 E A, dones
  // and rewards E (launch_rollout_w refuses a buffer whose bytes do not fit 32 bits)
  const unsigned nEO = (unsigned)E * (unsigned)O, nEA = (unsigned)E * (unsigned)A;

  for (int t = 0; t < a.T; ++t) {
    const long step_id = a.step0 + t;
    // tid, opaque to the compiler once per step (k_eval_w: the phases' index arithmetic does not depend
    // on the step; hoisted out of this loop it stays in VGPRs across layer 1, where W2 and the ring
    // leave it none)
    int td = tid;
    asm volatile("" : "+v"(td));
    // W1's first kRing k-blocks: their L2 round trip passes under the normalisation
    f4 ring[kRing][2];
    ring_fill<NTO, kRing>(ring, wsw, l1);
    // ---- normalised rows into XS (k_act3 order) ----
    for (int idx = td; idx < R * OP; idx += kActThreads) {
      const int r = idx / OP, f = idx - r * OP, e = row0 + r;
      const bool valid = e < E && f < O;
      const float x = valid ? XO[r * LDQ + f] : 0.0f;
      XS[r * LDX + f] = valid ? (x - NRM[f]) / NRM[OP + f] : x;
    }
    // ---- rollout stores of obs[t] / dones[t]: 32 lanes per env, one lane offset, in flight across the
    // barrier and layer 1 ----
    {
      const int r = td >> 5, i0 = td & 31, e = row0 + r;
      const PBuf so = step_buf(a.s_obs, t, nEO);
      const float* xo = XO + r * LDQ + i0;
      const unsigned off = ((unsigned)e * (unsigned)O + (unsigned)i0) * 4u;
      const int nv = e < E ? O - i0 : 0;  // this lane stores the dims 32 c + i0 with 32 c < nv
      float x[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) x[c] = xo[32 * c];  // inside the LDS row for every lane (LDQ > 32 NCH - 1)
#pragma unroll
      for (int c = 0; c < NCH; ++c) pst1(so, x[c], 32 * c < nv ? off + 128u * c : kDropped);
      const int de = row0 + (td & (R - 1));
      pst1(step_buf(a.s_dones, t, (unsigned)E), EV[EV_DONE * R + (td & (R - 1))], (td < R && de < E) ? (unsigned)de * 4u : kDropped);
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
    // the first Marsaglia-Tsang attempt's draws of this thread's first item do not depend on the
    // network; computed under layer 2's MFMAs (gamma_mt_d0 with them is gamma_mt, bitwise)
    GammaDraw gd0 = GammaDraw{0.f, 0.f};
    if (td < nitem) {
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
    // ---- concentrations and gamma draws (k_act3 stage 1); HP is dead, ITM takes its place ----
    for (int idx = td; idx < nitem; idx += kActThreads) {
      const BetaItem bi = beta_item(idx, A);
      const long env = row0 + bi.r;
      const float c = softplusf_(PRE[bi.r * LDP + bi.ai + bi.which * A]) + 1.0f;
      const float gs = idx == td ? gamma_mt_d0(c, gd0, key, env, step_id, bi.db) : gamma_mt(c, key, env, step_id, bi.db);
      float* it = ITM + idx * 4;  // ((r A + ai) 2 + which) 4
      it[0] = c;
      it[1] = gs;
    }
    lds_barrier();
    // ---- the action (stage 2) and its stores: actions[t], and (alpha, beta, sample)[t] for k_beta_logp ----
    for (int idx = td; idx < R * A; idx += kActThreads) {
      const int r = idx / A, ai = idx - r * A, e = row0 + r;
      const float* ia = ITM + (idx * 2 + 0) * 4;
      const float* ib = ITM + (idx * 2 + 1) * 4;
      const float al = ia[0], be = ib[0];
      const float s01 = beta_sample01(ia[1], ib[1]);
      const float act = beta_action(s01, lo, hi);
      ACT[r * 24 + ai] = act;
      if (e < E) {
        const unsigned ea = (unsigned)e * (unsigned)A + (unsigned)ai;
        pst1(step_buf(a.s_actions, t, nEA), act, ea * 4u);
        pst3(step_buf(a.s_beta, t, 3u * nEA), al, be, s01, ea * 12u);
      }
    }
    lds_barrier();
    // ---- env step: 32 lanes per env, NCH dims each (k_synth_step_wide's arithmetic); lane 0 stores
    // rewards[t] and keeps the next step's done ----
    {
      const int r = td >> 5, i0 = td & 31, e = row0 + r;
      if (e < E) {
        chee_lanes_step<R, NCH>(EV, r, i0, O, A, Q + r * LDQ, XO + r * LDQ, ACT + r * 24, a.lo, a.hi,
                                [&](const EnvLaneOut& o) {
                                  pst1(step_buf(a.s_rewards, t, (unsigned)E), o.reward, (unsigned)e * 4u);
                                  EV[EV_DONE * R + r] = o.fin ? 1.0f : 0.0f;
                                });
      }
    }
    lds_barrier();
  }
  // ---- epilogue: next_obs / next_done and the env state back to HBM ----
  env_slots_store<R, kActThreads>(EV, XO, Q, LDQ, sv, a.next_obs, a.next_done, row0, E, O, tid);
}

// 0 when k_rollout_w covers the agent: k_eval_w's set
int rollout_w_supported(const PackedLayout& K) { return eval_w_supported(K); }

// -1: the shape / env is not covered; -2: the LDS attribute; -6 (with a message): a rollout buffer too
// large for the kernel's 32-bit store offsets
int launch_rollout_w(const RolloutArgs& a, hipStream_t s) {
  if (rollout_w_supported(a.K) != 0 || a.env.w.on || a.env.kind != PSYN_CHEETAH || a.E <= 0 || a.T <= 0) return -1;
  if (!a.s_obs || !a.s_actions || !a.s_dones || !a.s_rewards || !a.s_beta) return -1;
  // the stores address a step's slice through a buffer resource: 32-bit byte offsets and range (k_upd2 has
  // the same rule at create). The largest buffers are obs [T][E][O] and (alpha, beta, sample) [T][E][A][3]
  const unsigned long long rows = (unsigned long long)a.T * a.E;
  const unsigned long long bytes = rows * 4ull * (unsigned long long)(a.K.O > 3 * a.K.A ? a.K.O : 3 * a.K.A);
  if (bytes >= kDropped)
    return ppo_fail("k_rollout_w: a rollout buffer of " + std::to_string(bytes) + " bytes (num_steps x num_envs = " +
                        std::to_string(rows) + " rows) does not fit the kernel's 32-bit store offsets; use fewer envs or "
                        "steps per context, or rollout=per_step",
                    -6);
  using GE = WideGeo<24, 3>;
  const size_t lds = (size_t)GE::total * sizeof(float);
  static const bool ok = hipFuncSetAttribute((const void*)k_rollout_w<24, 3, PSYN_CHEETAH>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
  if (!ok) return -2;
  hipLaunchKernelGGL((k_rollout_w<24, 3, PSYN_CHEETAH>), dim3((a.E + kRows - 1) / kRows), dim3(kActThreads), lds, s, a);
  return 0;
}
