// ppo_carla_conv.hip — the CaRL agent's forward convolutions (include/ppo_carla.h; reference
// include/carla/carla_model.h:222-318 with the carla_config.h defaults).
//
//  * k_conv: every convolution AND every Linear layer is one implicit GEMM on
//    mfma_f32_16x16x4f32 in the batch-on-lanes layout of the MLP kernels: a wave owns 16 output
//    pixels (flattened over samples and the output plane, so a Linear layer — a 1x1 "conv" on a
//    1x1 plane — tiles over samples) x 16·NOT output channels. The im2col offsets of the K = IC·k·k
//    reduction are a per-workgroup LDS table, so a B operand is one gathered load per lane and
//    k-step; A operands (weights [OC][IC·k·k]) stream from L2. The uint8 image is converted
//    (x / 255, carla_model.h:214-216, as x * (1/255): within 1 ulp) inside the first convolution's
//    gather.
//  * Concatenations are strides: conv6 and state_linear.2 write the two halves of the [n, 1280]
//    linear input, linear.2 writes the first 256 columns of the [n, 256 + NV] value-head input.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ppo_carla_units.hpp"

namespace {

constexpr int kConvWaves = 4;

// a wave: NP tiles of 16 output pixels x NOT tiles of 16 output channels
// Loads are unconditional from clamped addresses and masked with selects afterwards: a load under a
// per-lane branch is followed by its own s_waitcnt, which serialises the gather latency.
// The 4 waves of a workgroup share the output channels, so the weight tile of each 16-wide k group
// (16 NOT channels x 16 k) is loaded once per workgroup — coalesced, one float4 per thread and
// channel quarter — and staged in LDS in A-operand order: lane (j, g) of tile t reads its four
// k-steps as one ds_read_b128 (the per-wave scalar weight gathers read 16 rows x 16 B per
// instruction, 4 times over). Double-buffered, one barrier per k group; same operands and MFMA
// chain as before, so results are unchanged bit for bit.
template <int NOT, int NP, bool U8>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void k_conv(ConvArgs a) {
  __shared__ int koff[kMaxKTab + 4 * kUK];
  __shared__ __attribute__((aligned(16))) float wst[2][NOT * 256];  // [buf][t][g][j][st]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int KK = a.K * a.K, Kt = a.IC * KK, plane = a.IH * a.IW;
  for (int k = tid; k < Kt + 4 * kUK; k += 256) {  // padding: the last iteration reads without a branch
    const int ic = k / KK, rem = k - ic * KK, ky = rem / a.K, kx = rem - ky * a.K;
    koff[k] = k < Kt ? ic * plane + ky * a.IW + kx : 0;
  }
  const int P = a.OH * a.OW;
  const long Q = (long)a.n * P;
  // waves past the last pixel stay (masked) for the workgroup's staging and barriers
  const long q0 = ((long)blockIdx.x * kConvWaves + wave) * 16 * NP;
  // this lane's output pixels (B-operand column j of each pixel tile)
  long xbase[NP], obase[NP];
  bool qv[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    const long q = q0 + 16 * u + j;
    qv[u] = q < Q;
    const long s = qv[u] ? q / P : 0;
    const int p = qv[u] ? (int)(q - s * P) : 0, oy = p / a.OW, ox = p - oy * a.OW;
    xbase[u] = s * a.in_stride + (long)oy * a.S * a.IW + (long)ox * a.S;
    obase[u] = s * a.out_stride + p;
  }
  const int oc0 = blockIdx.y * 16 * NOT;
  f4 acc[NOT][NP];
#pragma unroll
  for (int t = 0; t < NOT; ++t)
#pragma unroll
    for (int u = 0; u < NP; ++u) acc[t][u] = f4{0.f, 0.f, 0.f, 0.f};
  const int kbeg = a.kc ? (int)blockIdx.z * a.kc : 0, kend = a.kc ? min(Kt, kbeg + a.kc) : Kt;
  // staging: thread (o = tid >> 2 + 64 h, c = tid & 3) owns channel oc0 + o, k-steps st = c: k0 + 4 c .. + 3
  // conv1 of a positional agent: its filters are wider than the IC image channels read here
  const int ws = U8 && a.wstride ? a.wstride : Kt;
  const bool vec = ((Kt | ws) & 3) == 0;  // rows start on 16-byte boundaries (uniform)
  constexpr int NH = (16 * NOT + 63) / 64;
  const int so = tid >> 2, sc = tid & 3;
  f4 wreg[NH];
  auto wload = [&](int k0) {
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int o = so + 64 * h, oc = oc0 + o, k = k0 + 4 * sc;
      const bool ocok = o < 16 * NOT && oc < a.OC;
      const float* row = a.W + (long)(ocok ? oc : 0) * ws;
      f4 v;
      if (vec) {
        v = *reinterpret_cast<const f4*>(row + min(k, Kt - 4));
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = row[min(k + i, Kt - 1)];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] *= (ocok && k + i < kend) ? 1.0f : 0.0f;
      wreg[h] = v;
    }
  };
  auto wstore = [&](int buf) {
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int o = so + 64 * h;
      if (o < 16 * NOT) {
        const int t = o >> 4, jj = o & 15;
#pragma unroll
        for (int i = 0; i < 4; ++i) wst[buf][((t * 4 + i) * 16 + jj) * 4 + sc] = wreg[h][i];
      }
    }
  };
  wload(kbeg);
  wstore(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kbeg; k0 < kend; k0 += 4 * kUK, buf ^= 1) {
    const bool more = k0 + 4 * kUK < kend;
    if (more) wload(k0 + 4 * kUK);
    float x[kUK][NP];
#pragma unroll
    for (int st = 0; st < kUK; ++st) {
      const int k = k0 + 4 * st + g;
      const bool kv = k < kend;
      const int ko = koff[k];
#pragma unroll
      for (int u = 0; u < NP; ++u) {
        const bool ok = kv && qv[u];
        const long off = ok ? xbase[u] + ko : 0;
        if constexpr (U8) {
          // unconditional load, masked as an integer; x / 255 as x * (1 / 255) (within 1 ulp of the
          // reference's division: a division sequence serialises the gather behind VCC); xscale is
          // 1 for a positional agent, whose reference never divides
          const int raw = a.in_u8[off];
          x[st][u] = (float)(ok ? raw : 0) * a.xscale;
        } else {
          x[st][u] = a.in_f[off] * (ok ? 1.0f : 0.0f);  // a multiplicative mask keeps the load unconditional
        }
      }
    }
    f4 w[NOT];  // w[t][st] = W[oc0 + 16 t + j][k0 + 4 st + g]
#pragma unroll
    for (int t = 0; t < NOT; ++t) w[t] = *reinterpret_cast<const f4*>(&wst[buf][(t * 64 + lane) * 4]);
#pragma unroll
    for (int st = 0; st < kUK; ++st)
#pragma unroll
      for (int t = 0; t < NOT; ++t)
#pragma unroll
        for (int u = 0; u < NP; ++u) acc[t][u] = mfma16(w[t][st], x[st][u], acc[t][u]);
    if (more) wstore(buf ^ 1);
    __syncthreads();
  }
  // lane (j, g) holds out channel oc0 + 16t + 4g + r of pixel q0 + 16u + j
  if (a.kc) {  // split K: raw partial sums, added in z order by k_conv_fin
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      if (!qv[u]) continue;
      float* o = a.part + ((size_t)blockIdx.z * Q + q0 + 16 * u + j) * a.OC;
#pragma unroll
      for (int t = 0; t < NOT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int oc = oc0 + 16 * t + 4 * g + r;
          if (oc < a.OC) o[oc] = acc[t][u][r];
        }
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    if (!qv[u]) continue;
    float* o = a.out + obase[u];
    int poy = 0, pox = 0;  // conv1 of a positional agent: this pixel's row and column
    if constexpr (U8) {
      if (a.rowb) {
        const long q = q0 + 16 * u + j;
        const int p = (int)(q - (q / P) * P);
        poy = p / a.OW;
        pox = p - poy * a.OW;
      }
    }
#pragma unroll
    for (int t = 0; t < NOT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int oc = oc0 + 16 * t + 4 * g + r;
        if (oc < a.OC) {
          float y = acc[t][u][r] + a.b[oc];
          if constexpr (U8) {
            if (a.rowb) y += a.rowb[oc * a.OH + poy] + a.colb[oc * a.OW + pox];
          }
          if (a.relu) y = y > 0.0f ? y : 0.0f;
          o[(long)oc * P] = y;
        }
      }
  }
}

// ---- conv2's forward from LDS-staged input patches (create option conv_fwd=tiled, the default) ----
// k_conv gathers each B operand from global memory (one load per MFMA for conv2's 16 output
// channels). Here a persistent workgroup walks TY x TX output tiles of one sample and stages the
// tile's input patch (IC x PH x PW, zero outside the plane) in LDS, the next tile's loaded into
// registers while the current one computes. GEMM: rows = oc (A = the weights, in registers for all
// tiles), columns = the tile's pixels (16 per MFMA column tile: one output row segment), k = (tap, ic)
// with k = 4 kk + g -> ic = 4 (kk % (IC / 4)) + g, tap = kk / (IC / 4): a lane's B operand is its
// pixel's patch offset + its ic plane + an IMMEDIATE per kk (ds_read_b32 + MFMA only). Same products as
// k_conv (fp32 MFMA), another k order (tolerance tests).
constexpr int kCtTY = 8, kCtTX = 16;  // conv2: 45 x 45 -> 6 x 3 tiles
template <int IC, int OC, int TY, int TX>
__global__ __launch_bounds__(256, 3) void k_conv_t(ConvArgs a, int tiles_x, int tps, int tiles) {
  constexpr int K = 5, S = 2, PH = (TY - 1) * S + K, PW = (TX - 1) * S + K, PP = PH * PW, NX = IC * PP;
  constexpr int NRT = OC / 16, ICQ = IC / 4, KS = K * K * ICQ, RPW = TY / 4, NSX = (NX + 255) / 256;
  static_assert(OC % 16 == 0 && IC % 4 == 0 && TY % 4 == 0 && TX == 16, "tile shape");
  __shared__ float xp[NX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  float wa[NRT][KS];  // A operands: W[16 rt + j][ic][tap], k = 4 kk + g
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int tap = kk / ICQ, ic = 4 * (kk - tap * ICQ) + g, oc = 16 * rt + j;
      wa[rt][kk] = a.W[(oc < a.OC ? oc * IC + ic : 0) * (K * K) + tap] * (oc < a.OC ? 1.0f : 0.0f);
    }
  float bias[NRT][4];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[rt][r] = a.b[16 * rt + 4 * g + r];
  const int bb = g * PP + S * RPW * wave * PW + S * j;  // + 4 (kk % ICQ) PP + ky PW + kx + S u PW
  const long plane = (long)a.IH * a.IW;
  const int P = a.OH * a.OW;
  float sx[NSX];
  auto sload = [&](int tile) {
    const int smp = tile / tps, tt = tile - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    const PBuf xb{__builtin_amdgcn_make_buffer_rsrc((void*)(a.in_f + (size_t)smp * a.in_stride), (short)0,
                                                    (int)(a.in_stride * 4), 0x00020000)};
    const int iy0 = S * TY * ty, ix0 = S * TX * tx;
#pragma unroll
    for (int i = 0; i < NSX; ++i) {
      const int e = tid + 256 * i, ic = e / PP, rem = e - ic * PP, r = rem / PW, c = rem - r * PW;
      const int iy = iy0 + r, ix = ix0 + c;
      const bool in = e < NX && iy < a.IH && ix < a.IW;
      const uint32_t off = in ? (uint32_t)(ic * plane + iy * a.IW + ix) * 4u : 0x7ffffff0u;
      sx[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xb.r, off, 0, 0));
    }
  };
  if ((int)blockIdx.x < tiles) sload(blockIdx.x);
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < NSX; ++i)
      if (tid + 256 * i < NX) xp[tid + 256 * i] = sx[i];
    __syncthreads();
    const int smp = tile / tps, tt = tile - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    if (tile + (int)gridDim.x < tiles) sload(tile + gridDim.x);
    f4 acc[NRT][RPW];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
      for (int u = 0; u < RPW; ++u) acc[rt][u] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int tap = kk / ICQ, icq = kk - tap * ICQ, ky = tap / K, kx = tap - ky * K;
      float bv[RPW];
#pragma unroll
      for (int u = 0; u < RPW; ++u) bv[u] = xp[bb + 4 * icq * PP + ky * PW + kx + S * u * PW];
#pragma unroll
      for (int u = 0; u < RPW; ++u)
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) acc[rt][u] = mfma16(wa[rt][kk], bv[u], acc[rt][u]);
      if (kk % 10 == 9) __builtin_amdgcn_sched_barrier(0);  // bounds the LDS read hoisting (registers)
    }
    __syncthreads();  // every wave is done with the patch before the next one is stored
    // lane (j, g) holds out channel 16 rt + 4 g + r of output pixel (TY ty + RPW wave + u, TX tx + j)
    const PBuf ob{__builtin_amdgcn_make_buffer_rsrc((void*)(a.out + (size_t)smp * a.out_stride), (short)0,
                                                    (int)(a.out_stride * 4), 0x00020000)};
    const int ox = TX * tx + j;
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
      for (int u = 0; u < RPW; ++u) {
        const int oy = TY * ty + RPW * wave + u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int oc = 16 * rt + 4 * g + r;
          const bool in = oy < a.OH && ox < a.OW && oc < a.OC;
          float y = acc[rt][u][r] + bias[rt][r];
          if (a.relu) y = y > 0.0f ? y : 0.0f;
          const uint32_t off = in ? (uint32_t)(oc * P + oy * a.OW + ox) * 4u : 0x7ffffff0u;
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y), ob.r, off, 0, 0);
        }
      }
  }
}

// ---- conv3's forward (IC 16, OC 32): k_conv_t with the two 16-channel row tiles on different waves ---
// 400 k x 32 rows of weights do not fit one wave's registers: wave w keeps row tile w & 1 (100 A
// operands) and takes half of the 8 x 8 output tile's pixels (two MFMA column tiles of 2 rows x 8
// columns). Patch rows PW = 24 floats (two output rows = 16 banks apart) and ic planes of odd length:
// a ds_read_b32 half (lane groups g = 0, 1) hits 32 distinct banks. k = 4 kk + g -> ic = 4 (kk % 4) + g,
// tap = kk / 4. Same products as k_conv (fp32 MFMA), another k order (tolerance tests).
constexpr int kCt2T = 8;  // output tile edge (conv3: 21 x 21 -> 3 x 3 tiles, 77 % used)
template <int IC, int OC>
__global__ __launch_bounds__(256, 2) void k_conv_t2(ConvArgs a, int tiles_x, int tps, int tiles) {
  constexpr int K = 5, S = 2, T = kCt2T, PH = (T - 1) * S + K, PWL = PH, PW = 24, PPA = 457, NXP = IC * PPA;
  constexpr int ICQ = IC / 4, KS = K * K * ICQ, NSX = (NXP + 255) / 256;
  static_assert(IC % 4 == 0 && OC == 32 && PW >= PWL && PPA >= PH * PW && (PPA & 1) && PW % 16 == 8, "shape");
  __shared__ float xp[NXP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int rt = wave & 1, ph = wave >> 1;
  float wa[KS];  // A operands: W[16 rt + j][ic][tap], k = 4 kk + g
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) {
    const int tap = kk / ICQ, ic = 4 * (kk - tap * ICQ) + g;
    wa[kk] = a.W[((16 * rt + j) * IC + ic) * (K * K) + tap];
  }
  float bias[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bias[r] = a.b[16 * rt + 4 * g + r];
  // lane j of column tile u: output pixel (2 (2 ph + u) + (j >> 3), j & 7) of the tile
  const int bb = g * PPA + 2 * (4 * ph + (j >> 3)) * PW + 2 * (j & 7);  // + 4 PW u + 4 (kk % ICQ) PPA + ky PW + kx
  const long plane = (long)a.IH * a.IW;
  const int P = a.OH * a.OW;
  float sx[NSX];
  auto sload = [&](int tile) {
    const int smp = tile / tps, tt = tile - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    const PBuf xb{__builtin_amdgcn_make_buffer_rsrc((void*)(a.in_f + (size_t)smp * a.in_stride), (short)0,
                                                    (int)(a.in_stride * 4), 0x00020000)};
    const int iy0 = S * T * ty, ix0 = S * T * tx;
#pragma unroll
    for (int i = 0; i < NSX; ++i) {
      const int e = tid + 256 * i, ic = e / PPA, rem = e - ic * PPA, r = rem / PW, c = rem - r * PW;
      const int iy = iy0 + r, ix = ix0 + c;
      const bool in = e < NXP && r < PH && c < PWL && iy < a.IH && ix < a.IW;
      const uint32_t off = in ? (uint32_t)(ic * plane + iy * a.IW + ix) * 4u : 0x7ffffff0u;
      sx[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xb.r, off, 0, 0));
    }
  };
  // no register prefetch of the next patch here (the weights take 100 VGPRs): the two workgroups of a
  // CU overlap one's staging with the other's MFMAs
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    sload(tile);
#pragma unroll
    for (int i = 0; i < NSX; ++i)
      if (tid + 256 * i < NXP) xp[tid + 256 * i] = sx[i];
    __syncthreads();
    const int smp = tile / tps, tt = tile - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    f4 acc[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int tap = kk / ICQ, icq = kk - tap * ICQ, ky = tap / K, kx = tap - ky * K;
      float bv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) bv[u] = xp[bb + 4 * PW * u + 4 * icq * PPA + ky * PW + kx];
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[u] = mfma16(wa[kk], bv[u], acc[u]);
      if (kk % 10 == 9) __builtin_amdgcn_sched_barrier(0);  // bounds the LDS read hoisting (registers)
    }
    __syncthreads();  // every wave is done with the patch before the next one is stored
    const PBuf ob{__builtin_amdgcn_make_buffer_rsrc((void*)(a.out + (size_t)smp * a.out_stride), (short)0,
                                                    (int)(a.out_stride * 4), 0x00020000)};
    const int ox = T * tx + (j & 7);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int oy = T * ty + 2 * (2 * ph + u) + (j >> 3);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int oc = 16 * rt + 4 * g + r;
        const bool in = oy < a.OH && ox < a.OW;
        float y = acc[u][r] + bias[r];
        if (a.relu) y = y > 0.0f ? y : 0.0f;
        const uint32_t off = in ? (uint32_t)(oc * P + oy * a.OW + ox) * 4u : 0x7ffffff0u;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y), ob.r, off, 0, 0);
      }
    }
  }
}

// split-K finish: out = relu(sum over z of the partials, in z order, + bias)
__global__ __launch_bounds__(256) void k_conv_fin(ConvArgs a, int Z) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int P = a.OH * a.OW;
  const long Q = (long)a.n * P;
  if (i >= Q * a.OC) return;
  const long q = i / a.OC;
  const int oc = (int)(i - q * a.OC);
  float v = 0.f;
  for (int z = 0; z < Z; ++z) v += a.part[(size_t)z * Q * a.OC + i];
  float y = v + a.b[oc];
  if (a.relu) y = y > 0.0f ? y : 0.0f;
  const long smp = q / P;
  a.out[smp * a.out_stride + (long)oc * P + (q - smp * P)] = y;
}

// ---- the first convolution (uint8 image, OC <= 16): input patch staged in LDS ----------------
// k_conv's gather issues one vector-memory byte load per lane, pixel tile and k-step (with the weight
// loads, 1.25 vector-memory instructions per MFMA), and conv1 — 15 x 25 taps per output pixel, most
// of the network's FLOPs — was bound by that instruction rate. Here a workgroup owns a 16 x 16 tile
// of output pixels of one sample (wave w: output rows 4w .. 4w + 3, lane j: column j): the
// (15 S + K)^2 x IC input patch is staged in LDS as bytes with aligned dword loads (~0.2 per MFMA),
// the weights and the im2col offsets are staged too, and every B operand is a ds_read_u8. The MFMA
// chain, the k order and the operands of every lane are those of k_conv: the outputs are bitwise
// equal (tested).
static size_t img_lds_bytes(int IC, int K, int S, int OC) {
  const int TI = (kImgTile - 1) * S + K, TIP = (TI + 3) & ~3, Kt = IC * K * K;
  const size_t patch = ((size_t)IC * TI * TIP + 15) & ~(size_t)15;
  return patch + (size_t)OC * (Kt + 64) * 4 + ((size_t)Kt + 64) * 4;
}

template <int K, int S>
__global__ __launch_bounds__(256) void k_conv_img(ConvArgs a) {
  using G = ImgGeo<K, S>;
  constexpr int TI = G::TI, TIP = G::TIP, DW = TIP / 4, UK = 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int KK = K * K, Kt = a.IC * KK, OC = a.OC;
  const size_t patch = ((size_t)a.IC * TI * TIP + 15) & ~(size_t)15;
  unsigned char* tile = smem;
  const int Ktp = Kt + 64;                                    // weight row pitch: zeros past Kt
  float* wl = reinterpret_cast<float*>(smem + patch);         // [OC][Ktp]
  int* koff = reinterpret_cast<int*>(wl + (size_t)OC * Ktp);  // [Ktp]: patch offset of tap k (0 past Kt)
  const int tiles_x = (a.OW + kImgTile - 1) / kImgTile;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x, smp = blockIdx.y;
  const int x0 = tx * kImgTile * S, y0 = ty * kImgTile * S;
  // patch rows: bytes [x0, x0 + TIP) of input rows y0 .. y0 + TI - 1 of every channel. Rows or
  // columns past the image read the next row / channel (or zeros past the buffer): they only reach
  // output pixels outside the image, which are not stored.
  {
    const unsigned char* base = a.in_u8 + (size_t)smp * a.in_stride;
    const size_t left = (size_t)(a.n - smp) * a.in_stride;
    const PBuf ib{__builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0,
                                                    (int)(left < 0xFFFFFFF0u ? left : 0xFFFFFFF0u), 0x00020000)};
    const int plane = a.IH * a.IW, total = a.IC * TI * DW;
    for (int e = tid; e < total; e += 256) {
      const int ic = e / (TI * DW), rem = e - ic * (TI * DW), r = rem / DW, d = rem - r * DW;
      const int off = ic * plane + (y0 + r) * a.IW + x0 + 4 * d;
      const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(ib.r, off, 0, 0);
      *reinterpret_cast<unsigned*>(tile + (ic * TI + r) * TIP + 4 * d) = v;
    }
  }
  for (int e = tid; e < OC * Ktp; e += 256) {
    const int oc = e / Ktp, k = e - oc * Ktp;
    wl[e] = k < Kt ? a.W[oc * (a.wstride ? a.wstride : Kt) + k] : 0.0f;
  }
  for (int k = tid; k < Kt + 64; k += 256) {
    const int ic = k / KK, rem = k - ic * KK, ky = rem / K, kx = rem - ky * K;
    koff[k] = k < Kt ? (ic * TI + ky) * TIP + kx : 0;
  }
  __syncthreads();
  int pix[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) pix[u] = S * (4 * wave + u) * TIP + S * j;
  const float* wrow = wl + (size_t)(j < OC ? j : 0) * Ktp;
  const float wm = j < OC ? 1.0f : 0.0f;
  f4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = f4{0.f, 0.f, 0.f, 0.f};
  // taps past Kt read offset 0 of the patch (a finite value) against a zero weight: the product is
  // +0, as k_conv's masked operands give, so no per-step masks are needed
  for (int k0 = 0; k0 < Kt; k0 += 4 * UK) {
    float x[UK][4], w[UK];
#pragma unroll
    for (int st = 0; st < UK; ++st) {
      const int k = k0 + 4 * st + g;
      const int ko = koff[k];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[st][u] = (float)tile[ko + pix[u]] * a.xscale;
      w[st] = wrow[k] * wm;
    }
#pragma unroll
    for (int st = 0; st < UK; ++st)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = mfma16(w[st], x[st][u], acc[u]);
  }
  const int P = a.OH * a.OW;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int oy = ty * kImgTile + 4 * wave + u, ox = tx * kImgTile + j;
    if (oy >= a.OH || ox >= a.OW) continue;
    float* o = a.out + (size_t)smp * a.out_stride + (size_t)oy * a.OW + ox;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int oc = 4 * g + r;
      if (oc < OC) {
        float y = acc[u][r] + a.b[oc];
        if (a.rowb) y += a.rowb[oc * a.OH + oy] + a.colb[oc * a.OW + ox];
        if (a.relu) y = y > 0.0f ? y : 0.0f;
        o[(size_t)oc * P] = y;
      }
    }
  }
}

// ---- conv1 with OC <= 8: two output columns per MFMA column --------------------------------
// With OC = 8, half of every 16-row A tile of k_conv_img is padding. Here A row oc + 8 dx holds the
// weights of channel oc shifted by dx output columns (S input columns) over an extended tap row
// kx' in [0, K + S): row oc + 8 dx, tap (ic, ky, kx') = W[oc][ic][ky][kx' - S dx] (0 outside the
// kernel), and lane column j of the B tile is output column 2 j, so one MFMA yields 16 output
// columns x 2 for all 8 channels. 15 x 5 x 7 = 525 taps per 32 outputs instead of 375 per 16:
// 31 % fewer MFMAs and LDS reads per output. The f32 MFMA accumulates like a sequential fma chain
// over k, the added taps carry exact zero weights (fma(+0, x >= 0, acc) = acc) and the real taps
// keep k_conv's order, so the outputs stay bitwise equal to k_conv's (tested).
constexpr int kImg2W = 32;  // output columns per workgroup tile
template <int K, int S>
struct Img2Geo {
  static constexpr int TI = (kImgTile - 1) * S + K;  // patch rows
  static constexpr int TW = (kImg2W - 1) * S + K;    // patch columns
  static constexpr int TIP = (TW + 3) & ~3;          // patch row pitch in bytes
  static constexpr int KX = K + S;                   // extended taps per kernel row
};
static size_t img2_lds_bytes(int IC, int K, int S, int OC) {
  const int TI = (kImgTile - 1) * S + K, TW = (kImg2W - 1) * S + K, TIP = (TW + 3) & ~3;
  const int Kt = IC * K * K, Kx = IC * K * (K + S);
  const size_t patch = ((size_t)IC * TI * TIP + 15) & ~(size_t)15;
  return patch + (size_t)OC * Kt * 4 + 2 * ((size_t)Kx + 64) * 4;
}

template <int K, int S>
__global__ __launch_bounds__(256) void k_conv_img2(ConvArgs a) {
  using G = Img2Geo<K, S>;
  constexpr int TI = G::TI, TIP = G::TIP, DW = TIP / 4, UK = 4, KX = G::KX;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int KK = K * K, Kt = a.IC * KK, Kx = a.IC * K * KX, OC = a.OC;
  const size_t patch = ((size_t)a.IC * TI * TIP + 15) & ~(size_t)15;
  unsigned char* tile = smem;
  float* wl = reinterpret_cast<float*>(smem + patch);         // [OC][Kt]
  int* poff = reinterpret_cast<int*>(wl + (size_t)OC * Kt);   // [Kx + 64]: patch offset of tap k'
  int* wtap = poff + Kx + 64;                                 // [Kx + 64]: (ic K + ky) K << 8 | kx'
  const int tiles_x = (a.OW + kImg2W - 1) / kImg2W;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x, smp = blockIdx.y;
  const int x0 = tx * kImg2W * S, y0 = ty * kImgTile * S;
  {  // the uint8 patch, as k_conv_img (bytes past the image only reach outputs that are not stored)
    const unsigned char* base = a.in_u8 + (size_t)smp * a.in_stride;
    const size_t left = (size_t)(a.n - smp) * a.in_stride;
    const PBuf ib{__builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0,
                                                    (int)(left < 0xFFFFFFF0u ? left : 0xFFFFFFF0u), 0x00020000)};
    const int plane = a.IH * a.IW, total = a.IC * TI * DW;
    for (int e = tid; e < total; e += 256) {
      const int ic = e / (TI * DW), rem = e - ic * (TI * DW), r = rem / DW, d = rem - r * DW;
      const int off = ic * plane + (y0 + r) * a.IW + x0 + 4 * d;
      const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(ib.r, off, 0, 0);
      *reinterpret_cast<unsigned*>(tile + (ic * TI + r) * TIP + 4 * d) = v;
    }
  }
  if (a.wstride) {  // a positional agent's wider filters: the image channels of each
    for (int e = tid; e < OC * Kt; e += 256) wl[e] = a.W[(e / Kt) * a.wstride + e % Kt];
  } else {
    for (int e = tid; e < OC * Kt; e += 256) wl[e] = a.W[e];
  }
  for (int k = tid; k < Kx + 64; k += 256) {
    const int ic = k / (K * KX), rem = k - ic * (K * KX), ky = rem / KX, kxp = rem - ky * KX;
    const bool in = k < Kx;
    poff[k] = in ? (ic * TI + ky) * TIP + kxp : 0;
    wtap[k] = in ? (((ic * K + ky) * K) << 8) | kxp : 255;  // kx' = 255: no tap (zero weight)
  }
  __syncthreads();
  int pix[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) pix[u] = S * (4 * wave + u) * TIP + 2 * S * j;
  const int aoc = j & 7, adx = j >> 3;  // A row j: channel aoc, shifted by adx output columns
  const bool aok = aoc < OC;
  const float* wrow = wl + (size_t)(aok ? aoc : 0) * Kt;
  f4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = f4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Kx; k0 += 4 * UK) {
    float x[UK][4], w[UK];
#pragma unroll
    for (int st = 0; st < UK; ++st) {
      const int k = k0 + 4 * st + g;
      const int po = poff[k], wt = wtap[k];
      const int kx = (wt & 255) - S * adx;
      const bool ok = aok && kx >= 0 && kx < K;
      const float wv = wrow[(wt >> 8) + min(max(kx, 0), K - 1)];
      w[st] = ok ? wv : 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u) x[st][u] = (float)tile[po + pix[u]] * a.xscale;
    }
#pragma unroll
    for (int st = 0; st < UK; ++st)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = mfma16(w[st], x[st][u], acc[u]);
  }
  // lane (j, g), register r: channel (4 g + r) & 7 of output column 2 j + ((4 g + r) >> 3)
  const int P = a.OH * a.OW;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int oy = ty * kImgTile + 4 * wave + u;
    if (oy >= a.OH) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ocp = 4 * g + r, oc = ocp & 7, ox = tx * kImg2W + 2 * j + (ocp >> 3);
      if (oc < OC && ox < a.OW) {
        float y = acc[u][r] + a.b[oc];
        if (a.rowb) y += a.rowb[oc * a.OH + oy] + a.colb[oc * a.OW + ox];
        if (a.relu) y = y > 0.0f ? y : 0.0f;
        a.out[(size_t)smp * a.out_stride + (size_t)oc * P + (size_t)oy * a.OW + ox] = y;
      }
    }
  }
}

// ---- conv1, packed taps (k_conv_img3; create option conv1=packed) -------------------------------
// k_conv_img2 spends 7.3 VALU and 1.6 LDS instructions per MFMA (SQ counters, profiles/r05/carla):
// every B operand is its own ds_read_u8 + convert + scale, every A operand an index lookup + select.
// Here the taps of one 16-wide MFMA k block are ordered so that lane group g's four k-steps are four
// CONSECUTIVE taps of one kernel row: tap (16 kb + 4 g + st) = extended column kx' = 4 (g & 1) + st of
// kernel row r = 2 kb + (g >> 1) (r = ic K + ky; kx' in [0, 8): k_conv_img2's K + S = 7 columns
// padded to 8 with a zero-weight tap). Then a lane's B operands for the four steps are the four bytes
// of ONE aligned dword of the patch row (ds_read_b32 + v_cvt_f32_ubyte0..3), and its A operands the
// four floats of one 16-byte piece of a pre-arranged weight table (wprep, built by k_conv1_wprep from
// W each call: A row i = oc + 8 dx holds W[oc][ic][ky][kx' - S dx], 0 outside the kernel), read from
// L2 one k block ahead. 38 blocks x 4 steps x 4 row tiles = 608 MFMAs per wave (k_conv_img2: 528) for
// ~8x fewer VALU and 5x fewer LDS instructions. Each product is k_conv's (x = u8 / 255, the same
// weight); only the order of the k chain differs (not bitwise k_conv's; tolerance tests).
constexpr int kImg3KX = 8;  // extended taps per kernel row, padded
template <int K, int S>
struct Img3Geo {
  static constexpr int TI = (kImgTile - 1) * S + K;          // patch rows
  static constexpr int TW = (kImg2W - 1) * S + K;            // patch columns used by real taps
  static constexpr int TIP = ((2 * S * (kImg2W / 2 - 1) + kImg3KX) + 3) & ~3;  // incl. the padding tap
};
static size_t img3_lds_bytes(int IC, int K, int S) {
  const int TI = (kImgTile - 1) * S + K, TIP = ((2 * S * (kImg2W / 2 - 1) + kImg3KX) + 3) & ~3;
  return ((size_t)IC * TI * TIP + 15) & ~(size_t)15;
}
// wprep[((kb * 4 + g) * 16 + i) * 4 + st] = A[i][tap 16 kb + 4 g + st]
// wstride: floats between two filters of W (IC K K, or more for a positional agent); xscale: the
// image's scale (1 / 255, or 1), folded into the weights
__global__ void k_conv1_wprep(const float* __restrict__ W, float* __restrict__ wp, int IC, int K, int S, int OC,
                              int nblk, int wstride, float xscale) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nblk * 256) return;
  const int st = e & 3, i = (e >> 2) & 15, g = (e >> 6) & 3, kb = e >> 8;
  const int r = 2 * kb + (g >> 1), kxp = 4 * (g & 1) + st;
  const int oc = i & 7, dx = i >> 3, kx = kxp - S * dx;
  float w = 0.0f;
  if (oc < OC && r < IC * K && kx >= 0 && kx < K) w = W[(size_t)oc * wstride + (size_t)r * K + kx];  // W[oc][ic][ky][kx]
  wp[e] = w * xscale;  // the image's 1 / 255 moves onto the weights: B is the raw byte value
}

// A workgroup walks tiles [t0, t1) (sample-major, 18 per 192 x 192 sample) with the A-operand table
// staged in LDS once (38 KB) and one patch buffer (35 KB), refilled per tile by LDS DMA (one dword a
// lane); two workgroups per CU, so one's patch fetch runs under the other's MFMAs. The k loop issues
// no vector-memory instruction: an A operand in global memory made the compiler wait vmcnt(0) at
// every k block (the ring index is not static), a full L2 round trip per 16 MFMAs.
constexpr int kImg3WG = 512;  // workgroups: two per CU
__host__ __device__ inline size_t img3_patch_bytes(int IC, int K, int S) {
  const int TI = (kImgTile - 1) * S + K, TIP = ((2 * S * (kImg2W / 2 - 1) + kImg3KX) + 3) & ~3;
  return ((size_t)IC * TI * TIP + 1023) & ~(size_t)1023;  // whole 4-wave DMA rounds (1 KB)
}
// BX (conv1_mfma=bx3): the k loop as v_mfma_f32_16x16x32_bf16 over block pairs (2 kk, 2 kk + 1): a
// lane's slots e < 4 are block 2 kk's taps st = e, slots 4 + st block 2 kk + 1's. The byte operands
// are exact bf16 numbers; the weights (fp32, 1/255 folded in) are split into their three pieces as
// they are read (split3_pair), so every product is exact and three 16-cycle MFMAs replace eight
// 32-cycle 16x16x4 f32 ones per row tile.
template <int K, int S, bool BX = false>
__global__ __launch_bounds__(256, 2) void k_conv_img3(ConvArgs a, int tiles, int tpc) {
  using G = Img3Geo<K, S>;
  constexpr int TI = G::TI, TIP = G::TIP, DW = TIP / 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int nblk = img3_blocks(a.IC, K), nrow = a.IC * K;
  const int pbytes = (int)img3_patch_bytes(a.IC, K, S), ndma = pbytes / 1024;  // DMA instructions per wave
  unsigned char* tile = smem;
  float* wl = reinterpret_cast<float*>(smem + pbytes);  // [nblk][4][16][4]
  const int tiles_x = (a.OW + kImg2W - 1) / kImg2W, tps = tiles_x * ((a.OH + kImgTile - 1) / kImgTile);
  const int t0 = blockIdx.x * tpc, t1 = min(tiles, t0 + tpc);
  if (t0 >= t1) return;
  for (int e = tid; e < nblk * 64; e += 256)
    reinterpret_cast<f4*>(wl)[e] = reinterpret_cast<const f4*>(a.wprep)[e];
  const int plane = a.IH * a.IW, total = a.IC * TI * DW;
  const float* wlane = wl + (g * 16 + j) * 4;  // this lane's piece of an A block
  const int P = a.OH * a.OW;
  int pix[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) pix[u] = S * (4 * wave + u) * TIP + 2 * S * j + 4 * (g & 1);
  // row 2 m + (g >> 1) of a ten-row step: channel (2 m + (g >> 1)) / K of the pair, kernel row % K
  int rowoff[5], rowq[5];
#pragma unroll
  for (int m = 0; m < 5; ++m) {
    const int rr = 2 * m + (g >> 1), q = rr / K, ky = rr - q * K;
    rowq[m] = q;
    rowoff[m] = (q * TI + ky) * TIP;
  }
  for (int t = t0; t < t1; ++t) {
    const int smp = t / tps, tt = t - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    __syncthreads();  // every wave is done with the previous tile's patch
    {  // wave w moves dwords (w ndma + q) 64 + lane of the patch, q < ndma
      const int x0 = tx * kImg2W * S, y0 = ty * kImgTile * S;
      const size_t sb = (size_t)smp * a.in_stride, left = (size_t)a.n * a.in_stride - sb;
      const PBuf ib{__builtin_amdgcn_make_buffer_rsrc((void*)(a.in_u8 + sb), (short)0,
                                                      (int)(left < 0xFFFFFFF0u ? left : 0xFFFFFFF0u), 0x00020000)};
      for (int q = 0; q < ndma; ++q) {
        const int e0 = (wave * ndma + q) * 64, e = e0 + lane;
        const int ic = e / (TI * DW), rem = e - ic * (TI * DW), r = rem / DW, d = rem - r * DW;
        const uint32_t voff = e < total ? (uint32_t)(ic * plane + (y0 + r) * a.IW + x0 + 4 * d) : 0xFFFFFFF0u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ib.r, (__attribute__((address_space(3))) void*)(tile + 4 * e0), 4,
                                                 voff, 0, 0, 0);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    f4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = f4{0.f, 0.f, 0.f, 0.f};
    if constexpr (BX) {
      // ten blocks (four channels) per step: five block pairs whose row offsets are per-lane constants
      for (int c4 = 0; c4 < (nblk + 9) / 10; ++c4) {
#pragma unroll
        for (int h5 = 0; h5 < 5; ++h5) {
          const int kk = 5 * c4 + h5;
          if (2 * kk >= nblk) break;
          unsigned xb[2][4];
          f4 wv[2];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int mm = 2 * h5 + t, c2 = 2 * c4 + (mm >= 5 ? 1 : 0), m = mm >= 5 ? mm - 5 : mm;
            const unsigned char* cbase = tile + (size_t)min(2 * c2, a.IC - 1) * TI * TIP;
            const unsigned char* prow =
                (2 * c2 + 1 < a.IC || rowq[m] == 0) ? cbase + rowoff[m] : tile + rowoff[m] % (TI * TIP);
#pragma unroll
            for (int u = 0; u < 4; ++u) xb[t][u] = *reinterpret_cast<const unsigned*>(prow + pix[u]);
            wv[t] = *reinterpret_cast<const f4*>(wlane + (2 * kk + t) * 256);
          }
          u32x4 ah, amd, al;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            unsigned h, md, l;
            split3_pair(wv[w >> 1][2 * (w & 1)], wv[w >> 1][2 * (w & 1) + 1], h, md, l);
            ah[w] = h; amd[w] = md; al[w] = l;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            u32x4 b;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const unsigned x = xb[w >> 1][u], sh = 16 * (w & 1);
              b[w] = pack_bf16_exact((float)((x >> sh) & 255u), (float)((x >> (sh + 8)) & 255u));
            }
            acc[u] = mfma16bx(al, b, acc[u]);
            acc[u] = mfma16bx(amd, b, acc[u]);
            acc[u] = mfma16bx(ah, b, acc[u]);
          }
        }
      }
    } else
    // Five k blocks = ten kernel rows = two input channels per step: the patch offset of every row is
    // a per-lane constant plus 2 TI TIP per step (rows past the last channel read channel 0: their
    // weights are 0). The operands of block kb + 1 are read from LDS under block kb's MFMAs.
    for (int c2 = 0; c2 < (a.IC + 1) / 2; ++c2) {
      const unsigned char* cbase = tile + (size_t)min(2 * c2, a.IC - 1) * TI * TIP;
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        const int kb = 5 * c2 + m;
        if (kb >= nblk) break;
        const unsigned char* prow = (2 * c2 + 1 < a.IC || rowq[m] == 0) ? cbase + rowoff[m] : tile + rowoff[m] % (TI * TIP);
        unsigned xb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) xb[u] = *reinterpret_cast<const unsigned*>(prow + pix[u]);
        const f4 wv = *reinterpret_cast<const f4*>(wlane + kb * 256);
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[u] = mfma16(wv[st], (float)((xb[u] >> (8 * st)) & 255u), acc[u]);
      }
    }
    // lane (j, g), register r: channel (4 g + r) & 7 of output column 2 j + ((4 g + r) >> 3) (k_conv_img2's)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int oy = ty * kImgTile + 4 * wave + u;
      if (oy >= a.OH) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ocp = 4 * g + r, oc = ocp & 7, ox = tx * kImg2W + 2 * j + (ocp >> 3);
        if (oc < a.OC && ox < a.OW) {
          float y = acc[u][r] + a.b[oc];
          if (a.rowb) y += a.rowb[oc * a.OH + oy] + a.colb[oc * a.OW + ox];
          if (a.relu) y = y > 0.0f ? y : 0.0f;
          a.out[(size_t)smp * a.out_stride + (size_t)oc * P + (size_t)oy * a.OW + ox] = y;
        }
      }
    }
  }
}

}  // namespace

int launch_conv(const ConvArgs& a, hipStream_t s, int img, bool fin, int* z_out) {
  if (z_out) *z_out = 1;
  if (a.IC * a.K * a.K > kMaxKTab) return -1;
  if (img == 2 && a.wprep && a.in_u8 && ((uintptr_t)a.in_u8 & 3) == 0 && a.K == 5 && a.S == 2 && a.OC <= 8 &&
      a.IW % 4 == 0 && a.in_stride % 4 == 0 && a.OH <= 16 * 64 &&
      img3_patch_bytes(a.IC, a.K, a.S) + (size_t)img3_blocks(a.IC, a.K) * 1024 <= 80 * 1024) {
    const int nblk = img3_blocks(a.IC, a.K);
    hipLaunchKernelGGL(k_conv1_wprep, dim3((nblk * 256 + 255) / 256), dim3(256), 0, s, a.W, a.wprep, a.IC, a.K, a.S,
                       a.OC, nblk, a.wstride ? a.wstride : a.IC * a.K * a.K, a.xscale);
    const int tiles = ((a.OW + kImg2W - 1) / kImg2W) * ((a.OH + kImgTile - 1) / kImgTile) * a.n;
    const int grid = std::min(tiles, kImg3WG), tpc = (tiles + grid - 1) / grid;
    const size_t lds = img3_patch_bytes(a.IC, a.K, a.S) + (size_t)nblk * 256 * sizeof(float);
    // the launch condition caps lds at 80 KB: allow that once for every later context and channel count
    static const bool attr =
        hipFuncSetAttribute((const void*)k_conv_img3<5, 2, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            80 * 1024) == hipSuccess &&
        hipFuncSetAttribute((const void*)k_conv_img3<5, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            80 * 1024) == hipSuccess;
    if (!attr) return -2;
    if (a.bx)
      hipLaunchKernelGGL((k_conv_img3<5, 2, true>), dim3((tiles + tpc - 1) / tpc), dim3(256), lds, s, a, tiles, tpc);
    else
      hipLaunchKernelGGL((k_conv_img3<5, 2, false>), dim3((tiles + tpc - 1) / tpc), dim3(256), lds, s, a, tiles, tpc);
    return hipGetLastError() == hipSuccess ? 0 : -2;
  }
  if (img && a.in_u8 && ((uintptr_t)a.in_u8 & 3) == 0 && a.K == 5 && a.S == 2 && a.OC <= 8 && a.IW % 4 == 0 &&
      a.in_stride % 4 == 0 && a.OH <= 16 * 64 && img2_lds_bytes(a.IC, a.K, a.S, a.OC) <= 64 * 1024) {
    const int tiles = ((a.OW + kImg2W - 1) / kImg2W) * ((a.OH + kImgTile - 1) / kImgTile);
    hipLaunchKernelGGL((k_conv_img2<5, 2>), dim3(tiles, a.n), dim3(256), img2_lds_bytes(a.IC, a.K, a.S, a.OC), s, a);
    return 0;
  }
  if (img && a.in_u8 && ((uintptr_t)a.in_u8 & 3) == 0 && a.K == 5 && a.S == 2 && a.OC <= 16 && a.IW % 4 == 0 &&
      a.in_stride % 4 == 0 &&
      a.OH <= 16 * 64 && img_lds_bytes(a.IC, a.K, a.S, a.OC) <= 64 * 1024) {
    const int tiles = ((a.OW + kImgTile - 1) / kImgTile) * ((a.OH + kImgTile - 1) / kImgTile);
    hipLaunchKernelGGL((k_conv_img<5, 2>), dim3(tiles, a.n), dim3(256), img_lds_bytes(a.IC, a.K, a.S, a.OC), s, a);
    return 0;
  }
  if (img && a.tiled && a.in_f && a.K == 5 && a.S == 2 && a.IC == 8 && a.OC == 16 && a.in_stride < (1L << 29) &&
      a.out_stride < (1L << 29)) {
    const int tiles_x = (a.OW + kCtTX - 1) / kCtTX, tps = tiles_x * ((a.OH + kCtTY - 1) / kCtTY);
    const long tiles = (long)a.n * tps;
    if (tiles < (1L << 31)) {
      const int grid = (int)std::min<long>(tiles, 256L * 3);  // three workgroups per CU (167 VGPRs)
      hipLaunchKernelGGL((k_conv_t<8, 16, kCtTY, kCtTX>), dim3(grid), dim3(256), 0, s, a, tiles_x, tps, (int)tiles);
      return 0;
    }
  }
  if (img && a.tiled && a.in_f && a.K == 5 && a.S == 2 && a.IC == 16 && a.OC == 32 && a.in_stride < (1L << 29) &&
      a.out_stride < (1L << 29)) {
    const int tiles_x = (a.OW + kCt2T - 1) / kCt2T, tps = tiles_x * ((a.OH + kCt2T - 1) / kCt2T);
    const long tiles = (long)a.n * tps;
    if (tiles < (1L << 31)) {
      const int grid = (int)std::min<long>(tiles, 256L * 2);
      hipLaunchKernelGGL((k_conv_t2<16, 32>), dim3(grid), dim3(256), 0, s, a, tiles_x, tps, (int)tiles);
      return 0;
    }
  }
  const long Q = (long)a.n * a.OH * a.OW;
  // several pixel tiles per wave where there are pixels to spare (B-operand reuse of every weight
  // load), one where the layer is narrow (Linear layers, the last convolutions)
  const int np = Q >= 16L * 4 * 1024 ? 4 : 1;
  const unsigned gx = (unsigned)((Q + 16 * kConvWaves * np - 1) / (16 * kConvWaves * np));
  const bool u8 = a.in_u8 != nullptr;
  const int Z = (a.part && !u8) ? conv_split_z(a.IC * a.K * a.K, a.OH * a.OW) : 1;
  ConvArgs b = a;
  b.kc = Z > 1 ? kSplitKC : 0;
#define PPO_CONV_LAUNCH(NOT_, NP_)                                                                          \
  do {                                                                                                     \
    const dim3 grid(gx, (a.OC + 16 * NOT_ - 1) / (16 * NOT_), Z);                                          \
    if (u8) hipLaunchKernelGGL((k_conv<NOT_, NP_, true>), grid, dim3(256), 0, s, b);                        \
    else hipLaunchKernelGGL((k_conv<NOT_, NP_, false>), grid, dim3(256), 0, s, b);                          \
  } while (0)
  if (a.OC >= 64) {
    if (np == 4) PPO_CONV_LAUNCH(4, 4);
    else PPO_CONV_LAUNCH(4, 1);
  } else if (a.OC >= 32) {
    if (np == 4) PPO_CONV_LAUNCH(2, 4);
    else PPO_CONV_LAUNCH(2, 1);
  } else {
    if (np == 4) PPO_CONV_LAUNCH(1, 4);
    else PPO_CONV_LAUNCH(1, 1);
  }
#undef PPO_CONV_LAUNCH
  if (z_out) *z_out = Z;
  if (Z > 1 && fin) hipLaunchKernelGGL(k_conv_fin, dim3((unsigned)((Q * a.OC + 255) / 256)), dim3(256), 0, s, b, Z);
  return 0;
}
