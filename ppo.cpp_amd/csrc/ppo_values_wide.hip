// ppo_values_wide.hip — k_values_w: the batched critic pass of the AC agent (LayerNorm-Beta, H = 256) at
// Humanoid width, OP = 384 (O <= 384): values[i] = critic(obs[i]) for n contiguous rows of [n][O]
// observations. k_values (ppo_rollout.hip) ends at OP = 112, where a wave's W1 slice still fits in
// registers beside its W2 slice; k_act3's critic workgroups (ppo_act.hip) take 16 rows each and stream
// all of W1 and W2 from L2 again for every 16 rows.
//
// k_values's contract: one persistent launch of min(row blocks, CUs) workgroups of 512 threads, a
// workgroup walks the R-row blocks blockIdx.x, blockIdx.x + gridDim.x, ..., wave w owns the output
// features [32 w, 32 w + 32), rows >= n of the last block are neither read nor stored. The chain is
// k_act3<LN_BETA, 24, 3>'s critic, op for op (bias-initialised accumulators, k-blocks ascending and
// .x .y .z .w within a block, act_activate's LayerNorm exchanges, the head as MFMAs split-K over the
// waves, their partials summed over waves 0 .. 7 ascending, then + the head bias), so every value is
// bitwise the one ppo_get_value returns (tests/test_gpu_values_wide.py). k_act3 runs its critic in the
// NHT = 3 geometry; a head tile has its own accumulator, so tile 0's sum does not depend on the others.
//
// The geometry is this kernel's own ("k_values_w"):
//  * registers: the wave's W2 slice stays resident for the launch (16 k-blocks x 2 tiles, 128 VGPRs).
//    Its W1 slice (24 k-blocks x 2 tiles) streams from L2 once per pass through a ring of kValRing
//    k-blocks (ring_fill / layer1_ring, ppo_wide_common.hpp), and a pass is RT = 2 row tiles, R = 32 rows:
//    one ring load of a k-block feeds the MFMAs of both tiles, so W1's traffic per row is half k_act3's
//    and W2's is none. The ring's first fill of a pass is issued before the pass's rows are normalised
//    into LDS, so its round trip passes under that phase.
//  * the next block's raw rows (R x 384 / 512 = 24 floats per thread) are loaded one block ahead into
//    registers, as k_values does, but only once layer 1 is over: the ring is dead from there to the next
//    pass's fill, so the 24 registers come out of its 64 and the loads' round trip passes under layer
//    2's MFMAs. Beside the ring they are live only while the rows are normalised, when no accumulator
//    or B operand is. A second XS buffer in LDS was not needed.
//  * the loads go through one buffer resource per group of 4 rows, whose range ends with row n - 1:
//    the hardware returns 0 for the rows past n and for a block past the last, with no branch and no
//    address past the buffer. Thread tid holds the elements tid + 512 u of the block, u = 0 .. 23;
//    512 x 3 = 384 x 4, so element u + 3 is element u four rows further down and a thread has three lane
//    offsets in all.
//  * LDS: XS (32 x 388) and HB (32 x 260) share one region, as in WideGeo: every wave is past
//    act_activate's barriers before HB is written, and past layer 2's before the next pass's XS. SP has
//    the critic's six vectors and one 16-row head tile (the value row and 15 zero rows); HP keeps head
//    row 0's partial of each wave only, and thread r < 32 sums them straight into values[row0 + r], so
//    there is no PRE region. 82 752 B in all.
#include "ppo_wide_common.hpp"

namespace {

constexpr int kValRT = 2;    // row tiles per pass (a third tile's 8 accumulators and 4 B registers spill)
constexpr int kValRing = 8;  // k-blocks of W1 in flight per wave (profiles/values_wide/resource_usage.txt)

template <int NTO>
struct ValWGeo {
  static constexpr int H = 256, OP = NTO * 16, NHP = 16, R = 16 * kValRT;
  static constexpr int LDX = ((OP + 63) / 64) * 64 + 4;
  static constexpr int LDH = H + 4;
  static constexpr int NSP = 6 * H + NHP * H;
  static constexpr int nXS = R * LDX, nHB = R * LDH;
  static constexpr int oU = 0;                                // XS -> HB in turn
  static constexpr int oSP = oU + (nXS > nHB ? nXS : nHB);    // b1 g1 be1 b2 g2 be2, the head tile's 16 rows
  static constexpr int oHBIAS = oSP + NSP;
  static constexpr int oRED = oHBIAS + NHP;                   // LayerNorm row sums, 2 x 8 x R
  static constexpr int oHP = oRED + 2 * kActWaves * R;        // head row 0's partials, 8 x R
  static constexpr int oNRM = oHP + kActWaves * R;            // obs mean | std (OP each)
  static constexpr int total = oNRM + 2 * OP;
  static constexpr int sB1 = 0, sG1 = H, sBE1 = 2 * H, sB2 = 3 * H, sG2 = 4 * H, sBE2 = 5 * H, sW3 = 6 * H;
  static_assert(oSP % 4 == 0 && LDX % 4 == 0 && LDH % 4 == 0, "f4 accesses of XS / HB / SP");
  static_assert((R * OP) % (3 * kActThreads) == 0 && (3 * kActThreads) % OP == 0, "three lane offsets per thread");
  static_assert(total * sizeof(float) <= 160 * 1024, "ValWGeo: the LDS carve exceeds a CU's 160 KB");
};

// a lane offset past the range of every row group's resource (at most 4 x 384 x 4 bytes): the load returns 0
constexpr unsigned kNoElem = 0xFFFFFF00u;

}  // namespace

template <int NTO>
__global__ __launch_bounds__(512) void k_values_w(ValuesArgs a) {
  using GE = ValWGeo<NTO>;
  constexpr int H = GE::H, OP = GE::OP, LDX = GE::LDX, LDH = GE::LDH, R = GE::R, RT = kValRT;
  constexpr int NXI = R * OP / kActThreads;       // raw obs elements per thread and block
  constexpr int DR = 3 * kActThreads / OP;        // rows between element u and element u + 3
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* XS = lds + GE::oU;
  float* HB = lds + GE::oU;
  float* SP = lds + GE::oSP;
  float* HBIAS = lds + GE::oHBIAS;
  float* RED = lds + GE::oRED;
  float* HP = lds + GE::oHP;
  float* NRM = lds + GE::oNRM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const PackedLayout& K = a.K;
  const float* __restrict__ P = a.P;
  const PBuf pb = make_pbuf(P, K.size);
  const int O = K.O;
  const long nblk = (a.n + R - 1) / R;

  // ---- prologue: W2 resident, staged parameters, the first block's rows ----
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
  stage_params<GE::NHP>(K, K.tr[0], pb, 0, SP, HBIAS, tid);
  for (int f = tid; f < OP; f += kActThreads) {
    NRM[f] = f < O ? P[K.omean + f] : 0.0f;
    NRM[OP + f] = f < O ? P[K.ostd + f] : 1.0f;
  }
  // block b's raw rows, element tid + 512 u in xnext[u]; rows >= n, dims >= O and a block >= nblk give 0
  float xnext[NXI];
  auto load_obs = [&](long b, int td) {
    const long row0 = b * R;
#pragma unroll
    for (int q = 0; q < NXI / 3; ++q) {
      // rows row0 + DR q .. + DR - 1 as one resource that ends with row n - 1; wave-uniform
      const long left = a.n - (row0 + DR * q);
      const int nrow = left < 0 ? 0 : left < DR ? (int)left : DR;
      const PBuf ob = make_pbuf(a.obs + (row0 + DR * q) * O, nrow * O);
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const int idx = td + kActThreads * v, r = idx / OP, f = idx - r * OP;
        const unsigned off = f < O ? (unsigned)(r * O + f) * 4u : kNoElem;
        xnext[3 * q + v] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ob.r, (int)off, 0, 0));
      }
    }
  };
  load_obs(blockIdx.x, tid);
  lds_barrier();  // SP / HBIAS / NRM staged

  for (long b = blockIdx.x; b < nblk; b += gridDim.x) {
    const long row0 = b * R;
    // tid, opaque to the compiler once per pass (k_eval_w: the index arithmetic of the phases that use it
    // does not depend on the pass; hoisted out of this loop it stays in VGPRs across layer 1, where W2,
    // the ring and two tiles' accumulators leave it none)
    int td = tid;
    asm volatile("" : "+v"(td));
    // W1's first kValRing k-blocks: their L2 round trip passes under the normalisation
    f4 ring[kValRing][2];
    ring_fill<NTO, kValRing>(ring, wsw, l1);
    // ---- normalised rows into XS (k_act3 order); every wave is past the previous pass's layer 2 (HB) ----
#pragma unroll
    for (int u = 0; u < NXI; ++u) {
      const int idx = td + kActThreads * (u % 3), r = idx / OP + DR * (u / 3), f = idx - (idx / OP) * OP;
      const bool valid = row0 + r < a.n && f < O;
      const float x = xnext[u];
      XS[r * LDX + f] = valid ? (x - NRM[f]) / NRM[OP + f] : x;
    }
    lds_barrier();
    // ---- layer 1 (W1 through the ring, both row tiles per k-block), LayerNorm + ReLU ----
    f4 acc[2][RT];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const f4 b1 = *reinterpret_cast<const f4*>(SP + GE::sB1 + 32 * wave + 16 * u + 4 * g);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[u][rt] = b1;
    }
    layer1_ring<NTO, kValRing, 16 * LDX>(acc, ring, wsw, l1, XS + j * LDX + 4 * g);
    act_activate<PPO_NET_LN_BETA, RT>(acc, SP + GE::sG1, SP + GE::sBE1, RED, wave, j, g);
    // every wave is past act_activate's barriers: XS is dead, HB takes its place
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
        *reinterpret_cast<f4*>(HB + (16 * rt + j) * LDH + 32 * wave + 16 * u + 4 * g) = acc[u][rt];
    lds_barrier();
    // ---- the next block's raw rows, in flight under layer 2 (the ring's registers are free) ----
    load_obs(b + gridDim.x, td);
    // ---- layer 2 (W2 resident), LayerNorm + ReLU ----
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const f4 b2 = *reinterpret_cast<const f4*>(SP + GE::sB2 + 32 * wave + 16 * u + 4 * g);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[u][rt] = b2;
    }
    const float* hin = HB + j * LDH + 4 * g;
    act_layer_regs<16, RT>(acc, w2, [&](int kb, int rt) { return *reinterpret_cast<const f4*>(hin + 16 * rt * LDH + 16 * kb); });
    act_activate<PPO_NET_LN_BETA, RT>(acc, SP + GE::sG2, SP + GE::sBE2, RED, wave, j, g);
    // ---- head: split-K partials over this wave's 32 features, one tile; head row 0 is the value ----
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      f4 hp = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const f4 wv = *reinterpret_cast<const f4*>(SP + GE::sW3 + j * H + 32 * wave + 16 * u + 4 * g);
        hp = mfma16(wv.x, acc[u][rt].x, hp);
        hp = mfma16(wv.y, acc[u][rt].y, hp);
        hp = mfma16(wv.z, acc[u][rt].z, hp);
        hp = mfma16(wv.w, acc[u][rt].w, hp);
      }
      if (g == 0) HP[wave * R + 16 * rt + j] = hp[0];
    }
    lds_barrier();
    // waves 0 .. 7 ascending, then + the head bias: k_act3's (and trunk_rows') order. The next write of
    // HP is four barriers away.
    if (td < R && row0 + td < a.n) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < kActWaves; ++w) s += HP[w * R + td];
      a.values[row0 + td] = s + HBIAS[0];
    }
  }
}

// 0 when k_values_w covers the agent: the AC agent at H = 256, OP = 384 (any A: the critic has one head)
int values_w_supported(const PackedLayout& K) {
  return (K.kind == PPO_NET_LN_BETA && K.H == 256 && K.OP == 384) ? 0 : -1;
}

// -1: the shape is not covered or the arguments are empty; -2: the LDS attribute
int launch_values_w(const ValuesArgs& a, hipStream_t s) {
  if (values_w_supported(a.K) != 0 || a.n <= 0 || !a.obs || !a.values || !a.WSW) return -1;
  using GE = ValWGeo<24>;
  const size_t lds = (size_t)GE::total * sizeof(float);
  static const bool ok = hipFuncSetAttribute((const void*)k_values_w<24>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds) == hipSuccess;
  if (!ok) return -2;
  const long nblk = (a.n + GE::R - 1) / GE::R;
  int dev = 0, ncu = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  const long grid = nblk < ncu ? nblk : ncu;  // one resident workgroup per CU (registers hold W2)
  hipLaunchKernelGGL((k_values_w<24>), dim3((unsigned)grid), dim3(kActThreads), lds, s, a);
  return 0;
}
