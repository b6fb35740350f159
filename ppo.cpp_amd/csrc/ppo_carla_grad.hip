// ppo_carla_grad.hip — the CaRL agent's backward through its convolution and Linear layers.
//
// Every convolution and Linear layer uses two kernels, both MFMA 16x16x4 in the
// batch-on-lanes layout of k_conv:
//  * k_dgrad — gradient w.r.t. the layer input, times the ReLU mask of that input (the previous
//    layer's output): a gather-GEMM over (output channel, tap). A strided convolution's input
//    pixels split into S x S parity classes (blockIdx.z); within a class the contributing taps are
//    a fixed set (ky = py + S*j), so the reduction has no zero-stuffed taps.
//  * k_wgrad — dW = dZ^T · im2col(x) with the bias as an extra all-ones column, split over
//    chunks of output pixels (blockIdx.x); k_wsum adds the chunks in order (deterministic).
// Linear layers are 1x1 convolutions on a 1x1 plane, as in the forward.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ppo_carla_units.hpp"

namespace {

constexpr int kMaxDTab = 3072;

template <int NOT, int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void k_dgrad(DgradArgs a) {
  __shared__ int woff[kMaxDTab + 4 * kUK], zoff[kMaxDTab + 4 * kUK];
  __shared__ int dji[kMaxDTab + 4 * kUK];
  __shared__ __attribute__((aligned(16))) float wst[2][NOT * 256];  // staged weights, as in k_conv
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int S = a.S, K = a.K, KK = K * K;
  const int py = blockIdx.z / S, px = blockIdx.z - py * S;
  const int nj = (K - py + S - 1) / S, ni = (K - px + S - 1) / S;
  const int OP = a.OH * a.OW, Kt = a.OC * nj * ni;
  for (int k = tid; k < Kt + 4 * kUK; k += 256) {  // padding entries (valid offsets) for the last iteration
    const int oc = k / (nj * ni), rem = k - oc * nj * ni, jj = rem / ni, ii = rem - jj * ni;
    const bool in = k < Kt;
    woff[k] = in ? oc * a.w_ic * KK + (py + S * jj) * K + (px + S * ii) : 0;
    zoff[k] = in ? oc * OP - jj * a.OW - ii : 0;
    dji[k] = in ? (jj << 16) | ii : 0;
  }
  __syncthreads();
  const int H2 = (a.IH - py + S - 1) / S, W2 = (a.IW - px + S - 1) / S, P2 = H2 * W2;
  const long Q = (long)a.n * P2;
  const long q0 = ((long)blockIdx.x * 4 + wave) * 16 * NP;  // waves past Q stay (masked) for the staging
  long zb[NP], sv[NP];
  int pix[NP], iy2v[NP], ix2v[NP];
  bool qv[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    const long q = q0 + 16 * u + j;
    qv[u] = q < Q;
    const long s = qv[u] ? q / P2 : 0;
    const int p2 = qv[u] ? (int)(q - s * P2) : 0, iy2 = p2 / W2, ix2 = p2 - iy2 * W2;
    sv[u] = s;
    iy2v[u] = iy2;
    ix2v[u] = ix2;
    zb[u] = s * a.dz_stride + (long)iy2 * a.OW + ix2;
    pix[u] = (S * iy2 + py) * a.IW + (S * ix2 + px);
  }
  const int ic0 = blockIdx.y * 16 * NOT;
  f4 acc[NOT][NP];
#pragma unroll
  for (int t = 0; t < NOT; ++t)
#pragma unroll
    for (int u = 0; u < NP; ++u) acc[t][u] = f4{0.f, 0.f, 0.f, 0.f};
  // weight tile of each k group (16 NOT input channels x 16 (oc, tap) entries) gathered once per
  // workgroup into LDS in A-operand order (k_conv's scheme): thread (o, c) loads k0 + 4 c .. + 3
  constexpr int NH = (16 * NOT + 63) / 64;
  const int so = tid >> 2, sc = tid & 3;
  float wreg[NH][4];
  auto wload = [&](int k0) {
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int o = so + 64 * h, ic = ic0 + o;
      const bool icok = o < 16 * NOT && ic < a.IC;
      const float* wr = a.W + (long)(icok ? ic : 0) * KK;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = k0 + 4 * sc + i;
        wreg[h][i] = wr[woff[k]] * ((icok && k < Kt) ? 1.0f : 0.0f);
      }
    }
  };
  auto wstore = [&](int buf) {
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int o = so + 64 * h;
      if (o < 16 * NOT) {
        const int t = o >> 4, jo = o & 15;
#pragma unroll
        for (int i = 0; i < 4; ++i) wst[buf][((t * 4 + i) * 16 + jo) * 4 + sc] = wreg[h][i];
      }
    }
  };
  wload(0);
  wstore(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < Kt; k0 += 4 * kUK, buf ^= 1) {
    const bool more = k0 + 4 * kUK < Kt;
    if (more) wload(k0 + 4 * kUK);
    float xb[kUK][NP];
#pragma unroll
    for (int st = 0; st < kUK; ++st) {
      const int k = k0 + 4 * st + g;
      const bool kv = k < Kt;
      const int zo = zoff[k], d = dji[k];
      const int jj = d >> 16, ii = d & 0xFFFF;
#pragma unroll
      for (int u = 0; u < NP; ++u) {
        const bool ok =
            kv && qv[u] && (unsigned)(iy2v[u] - jj) < (unsigned)a.OH && (unsigned)(ix2v[u] - ii) < (unsigned)a.OW;
        xb[st][u] = a.dz[ok ? zb[u] + zo : 0] * (ok ? 1.0f : 0.0f);
      }
    }
    f4 wa[NOT];  // wa[t][st] = W[oc(k)][ic0 + 16 t + j][tap(k)], k = k0 + 4 st + g
#pragma unroll
    for (int t = 0; t < NOT; ++t) wa[t] = *reinterpret_cast<const f4*>(&wst[buf][(t * 64 + lane) * 4]);
#pragma unroll
    for (int st = 0; st < kUK; ++st)
#pragma unroll
      for (int t = 0; t < NOT; ++t)
#pragma unroll
        for (int u = 0; u < NP; ++u) acc[t][u] = mfma16(wa[t][st], xb[st][u], acc[t][u]);
    if (more) wstore(buf ^ 1);
    __syncthreads();
  }
  const long plane = (long)a.IH * a.IW;
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    if (!qv[u]) continue;
#pragma unroll
    for (int t = 0; t < NOT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ic = ic0 + 16 * t + 4 * g + r;
        if (ic >= a.IC) continue;
        const float xm = a.x[sv[u] * a.x_stride + ic * plane + pix[u]];
        const float gv = xm > 0.0f ? acc[t][u][r] : 0.0f;
        float* o = a.dx + sv[u] * a.dx_stride + ic * plane + pix[u];
        *o = a.accumulate ? *o + gv : gv;
      }
  }
}

// ---- stride-2 input gradient with the dZ region staged in LDS (conv2: IC 8, OC 16, K 5) --------
// k_dgrad gathers every B operand (a dZ value) from global memory per lane and k-step. Here a
// workgroup owns a 32 x 32 block of input pixels of one sample: the OC x 18 x 18 dZ region those
// pixels read (zero outside the output plane) and the weights are staged in LDS. Wave w takes rows
// 4w .. 4w + 3 of each of the four parity classes (16 x 16 pixels each), so the 9-, 6-, 6- and
// 4-tap classes are spread evenly. Per class the k order (oc, jj, ii), the k-steps and each lane's
// operands are those of k_dgrad: the results are bitwise equal (tested).
constexpr int kDs2Tile = 32;                          // input pixels per block edge
constexpr int kDs2R = kDs2Tile / 2 + 2;               // dZ region edge for K = 5, S = 2
static size_t ds2_lds_bytes(int IC, int OC) {
  return ((size_t)OC * kDs2R * kDs2R + (size_t)OC * IC * 25 + 4 * 2 * (16 * 9 + 16)) * 4;
}

__global__ __launch_bounds__(256) void k_dgrad_s2(DgradArgs a, int tiles_x, int tps) {
  constexpr int K = 5, S = 2, KK = 25, R = kDs2R;
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int OC = a.OC, IC = a.IC, OP = a.OH * a.OW;
  float* dzl = dsm;                                // [OC][R][R]
  float* wl = dzl + OC * R * R;                    // W[oc][ic][K][K] of this layer (w_ic == IC)
  int* woff = reinterpret_cast<int*>(wl + OC * IC * KK);  // [4][16 * 9 + 16]
  int* zoff = woff + 4 * (16 * 9 + 16);
  const int smp = blockIdx.x / tps, tt = blockIdx.x - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
  const int oy0 = ty * (kDs2Tile / 2) - 2, ox0 = tx * (kDs2Tile / 2) - 2;  // dZ region origin
  {
    const float* dz = a.dz + (size_t)smp * a.dz_stride;
    for (int e = tid; e < OC * R * R; e += 256) {
      const int oc = e / (R * R), rem = e - oc * R * R, r = rem / R, q = rem - r * R;
      const int oy = oy0 + r, ox = ox0 + q;
      const bool in = (unsigned)oy < (unsigned)a.OH && (unsigned)ox < (unsigned)a.OW;
      const float v = dz[in ? (size_t)oc * OP + oy * a.OW + ox : 0];
      dzl[e] = in ? v : 0.0f;
    }
    for (int e = tid; e < OC * IC * KK; e += 256) wl[e] = a.W[e];
    for (int e = tid; e < 4 * (16 * 9 + 16); e += 256) {
      const int c = e / (16 * 9 + 16), k = e - c * (16 * 9 + 16), py = c >> 1, px = c & 1;
      const int nj = (K - py + S - 1) / S, ni = (K - px + S - 1) / S, Kt = OC * nj * ni;
      const int oc = k / (nj * ni), rem = k - oc * nj * ni, jj = rem / ni, ii = rem - jj * ni;
      const bool in = k < Kt;
      woff[e] = in ? oc * IC * KK + (py + S * jj) * K + (px + S * ii) : 0;
      zoff[e] = in ? oc * R * R - jj * R - ii : 0;
    }
  }
  __syncthreads();
  const int icr = j < IC ? j : 0;
  const float wm = j < IC ? 1.0f : 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int py = c >> 1, px = c & 1;
    const int nj = (K - py + S - 1) / S, ni = (K - px + S - 1) / S, Kt = OC * nj * ni;
    const int* wo_c = woff + c * (16 * 9 + 16);
    const int* zo_c = zoff + c * (16 * 9 + 16);
    // class-local pixel (ly, lx) = (4 wave + u, j): dZ row ly + 2 - jj, column lx + 2 - ii
    int zb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) zb[u] = (4 * wave + u + 2) * R + j + 2;
    f4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = f4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Kt; k0 += 4 * kUK) {
      float xb[kUK][4], wa[kUK];
#pragma unroll
      for (int st = 0; st < kUK; ++st) {
        const int k = k0 + 4 * st + g;
        const bool kv = k < Kt;
        const int wo = wo_c[k], zo = zo_c[k];
#pragma unroll
        for (int u = 0; u < 4; ++u) xb[st][u] = dzl[zb[u] + zo] * (kv ? 1.0f : 0.0f);
        wa[st] = wl[icr * KK + wo] * (kv ? wm : 0.0f);
      }
#pragma unroll
      for (int st = 0; st < kUK; ++st)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = mfma16(wa[st], xb[st][u], acc[u]);
    }
    const long plane = (long)a.IH * a.IW;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int iy = ty * kDs2Tile + S * (4 * wave + u) + py, ix = tx * kDs2Tile + S * j + px;
      if (iy >= a.IH || ix >= a.IW) continue;
      const long pix = (long)iy * a.IW + ix;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ic = 4 * g + r;
        if (ic >= IC) continue;
        const float xm = a.x[smp * a.x_stride + ic * plane + pix];
        const float gv = xm > 0.0f ? acc[u][r] : 0.0f;
        float* o = a.dx + smp * a.dx_stride + ic * plane + pix;
        *o = a.accumulate ? *o + gv : gv;
      }
    }
  }
}

// ---- conv2's input gradient as ONE GEMM over the four parity classes (create option
// conv_dgrad=quad, the default) --------------------------------------------------------------------
// For S = 2, K = 5 the input pixel (2 qy + py, 2 qx + px) of "quad" (qy, qx) reads dZ at
// (qy - jj, qx - ii), jj, ii < 3, through the tap (py + 2 jj, px + 2 ii), which does not exist when a
// coordinate is 5: all four parity classes of a quad read the SAME 3 x 3 dZ neighbourhood. So the
// classes become columns: rows = quads (16 per MFMA tile), k = (tap, oc) (9 x OC; a class's missing
// taps are zero weights), columns = (class, ic) — 4 x IC = 32 for IC = 8, two full 16-wide tiles,
// where k_dgrad_s2 leaves half of every MFMA's rows on IC = 8's padding to 16. 72 MFMAs per 16 quads
// (k_dgrad_s2: 100 with half the rows idle). A lane's A operand (dZ) is its quad's neighbourhood in
// the LDS-staged dZ region at one base address plus an IMMEDIATE offset per k-step (k = 4 kk + g:
// oc = 4 (kk % (OC / 4)) + g, tap kk / (OC / 4)), so the k loop is ds_read_b32 + MFMA only; the B
// operands (weights, 72 per lane) stay in registers for all tiles of the persistent workgroup. The
// next tile's dZ region is loaded into registers while the current one computes. Epilogue: the
// two px-classes of a quad sit in lanes j and j ^ 8, one exchange gives each lane four consecutive
// input pixels (two 8-byte stores, the ReLU mask read the same way). The sum runs in another order
// than k_dgrad's (tolerance tests, not bitwise).
constexpr int kDqT = 16;          // quads per tile row (32 input pixels)
constexpr int kDqU = 2;           // quad rows per wave: a tile is 4 kDqU x kDqT quads
constexpr int kDqR = kDqT + 2;    // dZ region row length (ii < 3)
template <int IC, int OC>
__global__ __launch_bounds__(256, kDqU == 2 ? 3 : 2) void k_dgrad_q(DgradArgs a, int tiles_x, int tps, int tiles) {
  constexpr int U = kDqU, TQY = 4 * U, RY = TQY + 2;
  constexpr int K = 5, R = kDqR, RR = RY * R, NCT = 4 * IC / 16, OCQ = OC / 4, KS = 9 * OCQ;
  // each oc plane padded to RRP = 16 (mod 32) dwords: lane groups g = 0, 1 (one ds_read_b32 half) read
  // 16 banks apart, conflict-free
  constexpr int RRP = ((RR - 16 + 31) / 32) * 32 + 16;
  constexpr int NST = (OC * RRP + 255) / 256;  // staging runs over the padded layout (linear LDS stores)
  static_assert(IC == 8 && OC % 4 == 0 && RRP >= RR, "the paired-lane epilogue is written for IC = 8");
  __shared__ float dzl[OC * RRP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int OP = a.OH * a.OW;
  // B operands: bw[ct][kk] = W[oc][ic][py + 2 jj][px + 2 ii] for column 16 ct + j = (class, ic), k = 4 kk + g
  float bw[NCT][KS];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int py = ct, px = j >> 3, ic = j & 7;  // IC = 8: column 16 ct + j = class (ct, j >> 3), channel j & 7
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int tap = kk / OCQ, oc = 4 * (kk - tap * OCQ) + g, ky = py + 2 * (tap / 3), kx = px + 2 * (tap % 3);
      const bool ok = ky < K && kx < K;
      bw[ct][kk] = ky < K ? a.W[((oc * IC + ic) * K + ky) * K + (ok ? kx : 0)] * (ok ? 1.0f : 0.0f) : 0.0f;
    }
  }
  // the lane's A base: dzl[g][4 wave][j]; step kk of row u adds 4 ocq RRP + (u + 2 - jj) R + (2 - ii)
  const int abase = g * RRP + U * wave * R + j;
  float st[NST];
  auto sload = [&](int tile) {
    const int smp = tile / tps, tt = tile - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    const int oy0 = ty * TQY - 2, ox0 = tx * kDqT - 2;
    // a buffer descriptor over the sample's dZ: elements outside the output plane read as 0 through an
    // offset past the buffer (no select after the load, so the loads stay in flight over the tile)
    const PBuf zb{__builtin_amdgcn_make_buffer_rsrc((void*)(a.dz + (size_t)smp * a.dz_stride), (short)0,
                                                    (int)(a.dz_stride * 4), 0x00020000)};
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int e = tid + 256 * i, oc = e / RRP, rem = e - oc * RRP, r = rem / R, q = rem - r * R;
      const int oy = oy0 + r, ox = ox0 + q;
      const bool in = e < OC * RRP && rem < RR && (unsigned)oy < (unsigned)a.OH && (unsigned)ox < (unsigned)a.OW;
      const uint32_t off = in ? (uint32_t)(oc * OP + oy * a.OW + ox) * 4u : 0x7ffffff0u;
      st[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(zb.r, off, 0, 0));
    }
  };
  if ((int)blockIdx.x < tiles) sload(blockIdx.x);
  const long plane = (long)a.IH * a.IW;
  const int px = j >> 3, icl = j & 7;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int e = tid + 256 * i;
      if (e < OC * RRP) dzl[e] = st[i];
    }
    __syncthreads();
    const int smp = tile / tps, tt = tile - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    if (tile + (int)gridDim.x < tiles) sload(tile + gridDim.x);
    f4 acc[U][NCT];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[u][ct] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int tap = kk / OCQ, ocq = kk - tap * OCQ, jj = tap / 3, ii = tap % 3;
      float av[U];
#pragma unroll
      for (int u = 0; u < U; ++u) av[u] = dzl[abase + 4 * ocq * RRP + (u + 2 - jj) * R + (2 - ii)];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
          if (ct + 2 * jj < K) acc[u][ct] = mfma16(av[u], bw[ct][kk], acc[u][ct]);  // py = 1 has no jj = 2 taps
      if (kk % 12 == 11) __builtin_amdgcn_sched_barrier(0);  // bounds the LDS read hoisting (registers)
    }
    __syncthreads();  // every wave is done with dzl before the next tile's region is stored
    // lane (j, g) holds, for quad row 4 wave + u and class (py = ct, px = j >> 3), channel j & 7 of the
    // quads 4 g + r; after the exchange with lane j ^ 8 it holds input pixels 8 g + 4 px + 0..3
    // the mask reads and the stores go through buffer descriptors: pixels past the plane read 0 and
    // their stores are dropped (an offset past the buffer), so there is no branch between the loads
    const PBuf xq{__builtin_amdgcn_make_buffer_rsrc((void*)(a.x + (size_t)smp * a.x_stride), (short)0,
                                                    (int)(a.x_stride * 4), 0x00020000)};
    const PBuf dq{__builtin_amdgcn_make_buffer_rsrc((void*)(a.dx + (size_t)smp * a.dx_stride), (short)0,
                                                    (int)(a.dx_stride * 4), 0x00020000)};
    const int ix = 2 * tx * kDqT + 8 * g + 4 * px;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const f4 v = acc[u][ct];
        const float s0 = px ? v[0] : v[2], s1 = px ? v[1] : v[3];
        const float r0 = __shfl_xor(s0, 8), r1 = __shfl_xor(s1, 8);
        const int iy = 2 * (ty * TQY + U * wave + u) + ct;
        float o[4];
        o[0] = px ? r0 : v[0];
        o[1] = px ? v[2] : r0;
        o[2] = px ? r1 : v[1];
        o[3] = px ? v[3] : r1;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bool in = iy < a.IH && ix + 2 * h < a.IW;
          const uint32_t off = in ? (uint32_t)(icl * plane + (long)iy * a.IW + ix + 2 * h) * 4u : 0x7ffffff0u;
          // (32-bit accesses; the compiler pairs the mask loads into one dwordx2)
          const float x0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xq.r, off, 0, 0));
          const float x1 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xq.r, off + 4, 0, 0));
          float g0 = x0 > 0.0f ? o[2 * h] : 0.0f;
          float g1 = x1 > 0.0f ? o[2 * h + 1] : 0.0f;
          if (a.accumulate) {
            g0 += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dq.r, off, 0, 0));
            g1 += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dq.r, off + 4, 0, 0));
          }
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, g0), dq.r, off, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, g1), dq.r, off + 4, 0, 0);
        }
      }
  }
}

// ---- conv3's input gradient (IC 16, OC 32): the quad form with the classes as separate GEMMs --------
// As k_dgrad_q, the four parity classes of a quad read the same 3 x 3 dZ neighbourhood, so one B
// operand (dZ at tap (jj, ii), oc = 4 ocq + g, from the LDS-staged region at a per-lane base plus an
// IMMEDIATE offset) feeds the MFMA of every class that has that tap. Here rows = the 16 input channels
// (full MFMA rows), columns = 16 quads (2 quad rows x 8 quad columns), and the A operands are the
// classes' weights from a table built once per persistent workgroup in LDS ([class k / 4][lane][4]:
// one ds_read_b128 per class and 4 k-steps); the classes' missing taps (py = 1: jj = 2, px = 1: ii = 2)
// are skipped: 200 MFMAs per wave and tile of 8 x 8 quads (conv3: 23 x 23 quads -> 3 x 3 tiles, 92 %
// used). Lane (j, g) ends with input channel 4 g + r of quad j for every class, so the px = 0 / 1
// classes of a row give two adjacent pixels. dZ region rows are 16 floats and oc planes 168 (= 8 mod 32):
// lane groups 0 and 1 read 32 distinct banks. Another sum order than k_dgrad (tolerance tests).
constexpr int kDq2T = 8;  // quads per tile edge
template <int IC, int OC>
__global__ __launch_bounds__(256, 2) void k_dgrad_q2(DgradArgs a, int tiles_x, int tps, int tiles) {
  constexpr int K = 5, R = 16, RU = kDq2T + 2, RRP = 168, OCQ = OC / 4, NTAB = (9 + 6 + 6 + 4) * OCQ * 64;
  constexpr int NST = (OC * RRP + 255) / 256;
  static_assert(IC == 16 && OC % 8 == 0 && RRP >= RU * R && RRP % 32 == 8, "shape");
  extern __shared__ __attribute__((aligned(16))) float dq2[];
  float* tab = dq2;          // [(class base + tap index * OCQ + ocq) / 4][lane][4]
  float* dzl = dq2 + NTAB;   // [OC][RRP]: rows of R
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  // class c = (py, px) = (c >> 1, c & 1): (3 - py) (3 - px) taps; k base (in k-steps) 0, 9, 15, 21 x OCQ
  auto cbase = [](int c) { return (c == 0 ? 0 : c == 1 ? 9 : c == 2 ? 15 : 21) * OCQ; };
  for (int f = tid; f < NTAB; f += 256) {
    const int e = f & 3, ln = (f >> 2) & 63, kc = 4 * (f >> 8) + e;
    const int c = kc < 9 * OCQ ? 0 : kc < 15 * OCQ ? 1 : kc < 21 * OCQ ? 2 : 3, py = c >> 1, px = c & 1;
    const int loc = kc - cbase(c), ti = loc / OCQ, ocq = loc - ti * OCQ, jj = ti / (3 - px), ii = ti - jj * (3 - px);
    const int oc = 4 * ocq + (ln >> 4), ic = ln & 15;
    tab[f] = a.W[((oc * IC + ic) * K + py + 2 * jj) * K + px + 2 * ii];
  }
  const int bbase = g * RRP + (2 * wave + (j >> 3)) * R + (j & 7);  // + 4 ocq RRP + (2 - jj) R + (2 - ii)
  const int OP = a.OH * a.OW;
  float st[NST];
  auto sload = [&](int tile) {
    const int smp = tile / tps, tt = tile - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    const int oy0 = ty * kDq2T - 2, ox0 = tx * kDq2T - 2;
    const PBuf zb{__builtin_amdgcn_make_buffer_rsrc((void*)(a.dz + (size_t)smp * a.dz_stride), (short)0,
                                                    (int)(a.dz_stride * 4), 0x00020000)};
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int e = tid + 256 * i, oc = e / RRP, rem = e - oc * RRP, r = rem / R, q = rem - r * R;
      const int oy = oy0 + r, ox = ox0 + q;
      const bool in = e < OC * RRP && r < RU && q < RU && (unsigned)oy < (unsigned)a.OH && (unsigned)ox < (unsigned)a.OW;
      const uint32_t off = in ? (uint32_t)(oc * OP + oy * a.OW + ox) * 4u : 0x7ffffff0u;
      st[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(zb.r, off, 0, 0));
    }
  };
  if ((int)blockIdx.x < tiles) sload(blockIdx.x);
  const long plane = (long)a.IH * a.IW;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < NST; ++i)
      if (tid + 256 * i < OC * RRP) dzl[tid + 256 * i] = st[i];
    __syncthreads();
    const int smp = tile / tps, tt = tile - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    if (tile + (int)gridDim.x < tiles) sload(tile + gridDim.x);
    f4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int jj = t / 3, ii = t % 3;
#pragma unroll
      for (int h = 0; h < OCQ / 4; ++h) {
        f4 wa[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int py = c >> 1, px = c & 1;
          if (jj < 3 - py && ii < 3 - px) {
            const int kk4 = (cbase(c) + (jj * (3 - px) + ii) * OCQ) / 4 + h;
            wa[c] = *reinterpret_cast<const f4*>(&tab[(kk4 * 64 + lane) * 4]);
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ocq = 4 * h + q;
          const float bv = dzl[bbase + 4 * ocq * RRP + (2 - jj) * R + (2 - ii)];
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (jj < 3 - (c >> 1) && ii < 3 - (c & 1)) acc[c] = mfma16(wa[c][q], bv, acc[c]);
        }
      }
    }
    __syncthreads();  // every wave is done with dzl before the next tile's region is stored
    // lane (j, g): channel 4 g + r of quad (2 wave + (j >> 3), j & 7) for class c; px = 0 / 1 adjacent
    const PBuf xq{__builtin_amdgcn_make_buffer_rsrc((void*)(a.x + (size_t)smp * a.x_stride), (short)0,
                                                    (int)(a.x_stride * 4), 0x00020000)};
    const PBuf dq{__builtin_amdgcn_make_buffer_rsrc((void*)(a.dx + (size_t)smp * a.dx_stride), (short)0,
                                                    (int)(a.dx_stride * 4), 0x00020000)};
    const int qy = ty * kDq2T + 2 * wave + (j >> 3), ix = 2 * (tx * kDq2T + (j & 7));
#pragma unroll
    for (int py = 0; py < 2; ++py) {
      const int iy = 2 * qy + py;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ic = 4 * g + r;
#pragma unroll
        for (int px = 0; px < 2; ++px) {
          const bool in = iy < a.IH && ix + px < a.IW;
          const uint32_t off = in ? (uint32_t)(ic * plane + (long)iy * a.IW + ix + px) * 4u : 0x7ffffff0u;
          const float xm = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xq.r, off, 0, 0));
          float gv = xm > 0.0f ? acc[2 * py + px][r] : 0.0f;
          if (a.accumulate) gv += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dq.r, off, 0, 0));
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, gv), dq.r, off, 0, 0);
        }
      }
    }
  }
}
static size_t dq2_lds_bytes(int OC) { return ((size_t)(9 + 6 + 6 + 4) * (OC / 4) * 64 + (size_t)OC * 168) * 4; }

// ---- the last convolution's input gradient as a dense GEMM + col2im (create option deep_dgrad=col) ----
// conv6 (4 x 4 -> 2 x 2, stride 1) has 4 output pixels: k_dgrad's per-pixel tap sets are mostly
// outside the output plane (2.25 of 9 taps valid on average, the rest multiply zeros). Instead dcol[n][(ic, ky, kx)][oy, ox] = sum_oc W[oc][ic, ky, kx] dZ[n][oc][oy, ox]
// is one dense GEMM (k_conv as a 1 x 1 convolution over the OH x OW plane with the transposed weights,
// no zero products), and k_col2im adds each input pixel's (at most K x K) contributions in (ky, kx)
// order and applies the ReLU mask. Another sum order than k_dgrad (tolerance tests).
__global__ void k_wtrans(const float* __restrict__ W, int OC, int Kt, float* __restrict__ Wt) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // Wt[k][oc] = W[oc][k]
  if (i >= (long)OC * Kt) return;
  const int k = (int)(i / OC), oc = (int)(i - (long)k * OC);
  Wt[i] = W[(long)oc * Kt + k];
}
template <int K, int S>
__global__ void k_col2im(const float* __restrict__ dcol, const float* __restrict__ x, long x_stride,
                         float* __restrict__ dx, long dx_stride, int IC, int IH, int IW, int OH, int OW, int n,
                         int accumulate) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)IC * IH * IW;
  if (i >= per * n) return;
  const long smp = i / per;
  const int r = (int)(i - smp * per), ic = r / (IH * IW), p = r - ic * IH * IW, iy = p / IW, ix = p - iy * IW;
  const int OP = OH * OW;
  const float* col = dcol + (size_t)smp * IC * K * K * OP + (size_t)ic * K * K * OP;
  float v = 0.0f;
#pragma unroll
  for (int ky = 0; ky < K; ++ky) {
    const int dy = iy - ky, oy = dy / S;
    if (dy < 0 || dy % S || oy >= OH) continue;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int dxx = ix - kx, ox = dxx / S;
      if (dxx < 0 || dxx % S || ox >= OW) continue;
      v += col[(ky * K + kx) * OP + oy * OW + ox];
    }
  }
  const float xm = x[smp * x_stride + r];
  const float gv = xm > 0.0f ? v : 0.0f;
  float* o = dx + smp * dx_stride + r;
  *o = accumulate ? *o + gv : gv;
}

constexpr int kMaxPTab = 9216;  // output pixels per sample (94 x 94 = 8836 for conv1)
constexpr uint32_t kWgradFar = 0x70000000u;  // k_wgrad's out-of-range byte offset (fp32 inputs stay below it)

template <int NOT, int NKT, bool U8>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void k_wgrad(WgradArgs a) {
  // U q-steps per iteration: all their loads are issued before their MFMAs (the narrow layers have
  // the longest pixel runs and the fewest MFMAs per load, so they get the deepest batch)
  constexpr int U = NOT == 1 ? 8 : 2;
  constexpr int NA = 16 * NOT * 4 * U;           // dZ tile of one iteration (channels x pixels)
  constexpr int NAT = (NA + 255) / 256;          // dZ elements staged per thread
  __shared__ int koff[kMaxKTab];
  __shared__ int pbase[kMaxPTab];
  __shared__ __attribute__((aligned(16))) float ast[2][NA];  // [buf][t][g][j][st]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int KK = a.K * a.K, plane = a.IH * a.IW;
  for (int k = tid; k < a.Kt; k += 256) {
    const int ic = k / KK, rem = k - ic * KK, ky = rem / a.K, kx = rem - ky * a.K;
    koff[k] = ic * plane + ky * a.IW + kx;
  }
  for (int p = tid; p < a.OP; p += 256) {
    const int oy = p / a.OW, ox = p - oy * a.OW;
    pbase[p] = oy * a.S * a.IW + ox * a.S;
  }
  const long Q = (long)a.n * a.OP;
  const long qs = (long)blockIdx.x * a.qchunk;
  const long qe = qs + a.qchunk < Q ? qs + a.qchunk : Q;
  const int oc0 = blockIdx.y * 16 * NOT;
  // waves whose columns start past Kt stay (their columns are masked) for the workgroup's staging
  const int kb = (blockIdx.z * 4 + wave) * 16 * NKT;
  f4 acc[NOT][NKT];
#pragma unroll
  for (int t = 0; t < NOT; ++t)
#pragma unroll
    for (int u = 0; u < NKT; ++u) acc[t][u] = f4{0.f, 0.f, 0.f, 0.f};
  int ko[NKT];
  int kc[NKT];  // 0: gathered column, 1: bias column, 2: past the end
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NKT; ++u) {
    const int k = kb + 16 * u + j;
    kc[u] = k < a.Kt ? 0 : (k == a.Kt ? 1 : 2);
    ko[u] = k < a.Kt ? koff[k] : 0;
  }
  // fp32 input: the gathers go through a buffer descriptor with 32-bit byte offsets (the whole
  // minibatch's activations are < 4 GB, launch condition): column byte offsets ko4 (a value far past
  // the buffer for the bias / padding columns) plus the pixel's byte offset xb4 (also far past the
  // buffer for pixels past the chunk), so a column reads 0 out of range instead of through a select
  // and 64-bit address arithmetic (round 5: 15 VALU per MFMA before, SQ counters)
  constexpr uint32_t kFar = kWgradFar;
  uint32_t ko4[NKT];
#pragma unroll
  for (int u = 0; u < NKT; ++u) ko4[u] = kc[u] == 0 ? (uint32_t)ko[u] * 4u : kFar;
  const PBuf xbuf{__builtin_amdgcn_make_buffer_rsrc((void*)(U8 ? (const void*)a.x_u8 : (const void*)a.x_f), (short)0,
                                                    (int)(U8 ? 0 : (uint32_t)min((long)a.n * a.x_stride * 4, (long)kFar)),
                                                    0x00020000)};
  // The dZ operand (the A side) is the same for the workgroup's 4 waves: each iteration's
  // 16 NOT x 4 U tile is loaded once per workgroup (element e = tid + 256 h: channel e / (4 U),
  // pixel qb + e % (4 U), consecutive threads on consecutive pixels) and staged in LDS in A-operand
  // order (lane (j, g) reads its U steps of tile t as one vector). Same operands and MFMA chain as
  // the per-wave gathers: bitwise unchanged.
  long as_[NAT];
  int ap_[NAT];
  auto apos = [&](int h, long q) {  // (sample, pixel) of pixel q for staging slot h
    const long sm = q / a.OP;
    as_[h] = sm;
    ap_[h] = (int)(q - sm * a.OP);
  };
#pragma unroll
  for (int h = 0; h < NAT; ++h) apos(h, qs + (tid + 256 * h) % (4 * U));
  float areg[NAT];
  auto aload = [&](long qb) {
#pragma unroll
    for (int h = 0; h < NAT; ++h) {
      const int e = tid + 256 * h, o = e / (4 * U), pi = e - o * (4 * U), oc = oc0 + o;
      const bool ok = e < NA && oc < a.OC && qb + pi < qe;
      areg[h] = a.dz[ok ? as_[h] * a.dz_stride + (long)oc * a.OP + ap_[h] : 0] * (ok ? 1.0f : 0.0f);
      // advance to the next iteration's pixel (qb + 4 U + pi)
      long sm = as_[h];
      int pp = ap_[h] + 4 * U;
      while (pp >= a.OP) {
        pp -= a.OP;
        ++sm;
      }
      as_[h] = sm;
      ap_[h] = pp;
    }
  };
  auto astore = [&](int buf) {
#pragma unroll
    for (int h = 0; h < NAT; ++h) {
      const int e = tid + 256 * h;
      if (e < NA) {
        const int o = e / (4 * U), pi = e - o * (4 * U), t = o >> 4, jo = o & 15, st = pi >> 2, gg = pi & 3;
        ast[buf][((t * 4 + gg) * 16 + jo) * U + st] = areg[h];
      }
    }
  };
  long q = qs + g;
  long s = q / a.OP;
  int p = (int)(q - s * a.OP);
  const bool wrap1 = a.OP >= 4;
  aload(qs);
  astore(0);
  __syncthreads();
  int buf = 0;
  for (long qb = qs; qb < qe; qb += 4 * U, buf ^= 1) {
    const bool more = qb + 4 * U < qe;
    if (more) aload(qb + 4 * U);
    float bv[U][NKT];
#pragma unroll
    for (int st = 0; st < U; ++st) {
      const bool qv = q < qe;
      if constexpr (U8) {
        const long xb = s * a.x_stride + (qv ? pbase[p] : 0);
#pragma unroll
        for (int u = 0; u < NKT; ++u) {
          const bool ok = qv && kc[u] == 0;
          const long off = ok ? xb + ko[u] : 0;
          const int raw = a.x_u8[off];
          const float v = (float)(ok ? raw : 0) * a.xscale;
          bv[st][u] = (qv && kc[u] == 1) ? 1.0f : v;
        }
      } else {
        const uint32_t xb4 = qv ? (uint32_t)(s * a.x_stride + pbase[p]) * 4u : kFar;
#pragma unroll
        for (int u = 0; u < NKT; ++u) {
          const float v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xbuf.r, xb4 + ko4[u], 0, 0));
          bv[st][u] = (qv && kc[u] == 1) ? 1.0f : v;
        }
      }
      q += 4;
      p += 4;
      if (wrap1) {  // OP >= 4: at most one sample boundary per step (branch-free)
        const bool w = p >= a.OP;
        p -= w ? a.OP : 0;
        s += w ? 1 : 0;
      } else {
        while (p >= a.OP) {
          p -= a.OP;
          ++s;
        }
      }
    }
    float av[NOT][U];  // av[t][st] = dZ[oc0 + 16 t + j][pixel qb + 4 st + g]
#pragma unroll
    for (int t = 0; t < NOT; ++t)
#pragma unroll
      for (int st = 0; st < U; ++st) av[t][st] = ast[buf][((t * 4 + g) * 16 + j) * U + st];
#pragma unroll
    for (int st = 0; st < U; ++st)
#pragma unroll
      for (int t = 0; t < NOT; ++t)
#pragma unroll
        for (int u = 0; u < NKT; ++u) acc[t][u] = mfma16(av[t][st], bv[st][u], acc[t][u]);
    if (more) astore(buf ^ 1);
    __syncthreads();
  }
  float* out = a.part + (long)blockIdx.x * a.OC * (a.Kt + 1);
#pragma unroll
  for (int t = 0; t < NOT; ++t)
#pragma unroll
    for (int u = 0; u < NKT; ++u) {
      const int k = kb + 16 * u + j;
      if (k > a.Kt) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int oc = oc0 + 16 * t + 4 * g + r;
        if (oc < a.OC) out[(long)oc * (a.Kt + 1) + k] = acc[t][u][r];
      }
    }
}

// ---- conv1's weight gradient (uint8 image, OC <= 16): input patch and dZ tile staged in LDS ----
// dW[oc][k] (+ the bias column k = Kt) = sum over output pixels of dZ[oc][px] * im2col(x)[px][k].
// k_wgrad gathers every B operand from global memory (a byte per lane and k-step): for conv1, with
// 18 M output pixels per 2 048-row minibatch, that instruction rate was the bound. Here workgroup c
// walks output tiles [c * tpc, (c + 1) * tpc) (16 x 16 pixels of one sample each); per tile the
// (15 S + K)^2 x IC uint8 patch and the OC x 256 dZ tile (zero outside the image) are staged in LDS,
// and wave w accumulates column tiles 6w .. 6w + 5 of the [OC] x [Kt + 1] product over the tile's
// 256 pixels (A = dZ, B = ds_read_u8 gathers), across all its tiles. Partials: part[c][OC][Kt + 1],
// reduced by k_wsum1 / k_wsum in chunk order as k_wgrad's.
constexpr int kWimgCT = 6;  // column tiles per wave: 4 waves x 6 x 16 = 384 >= Kt + 1 = 376
static size_t wimg_lds_bytes(int IC, int K, int S, int OC) {
  const int TI = (kImgTile - 1) * S + K, TIP = (TI + 3) & ~3;
  const size_t patch = ((size_t)IC * TI * TIP + 15) & ~(size_t)15;
  return patch + (size_t)OC * 260 * 4;
}

template <int K, int S>
__global__ __launch_bounds__(256) void k_wgrad_img(WgradArgs a, int tiles_x, int tps, int tiles, int tpc) {
  using G = ImgGeo<K, S>;
  constexpr int TI = G::TI, TIP = G::TIP, DW = TIP / 4, DZP = 260;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int KK = K * K, Kt = a.Kt, OC = a.OC, plane = a.IH * a.IW;
  const size_t patch = ((size_t)a.IC * TI * TIP + 15) & ~(size_t)15;
  unsigned char* tile = smem;
  float* dzl = reinterpret_cast<float*>(smem + patch);  // [OC][DZP]: pixel 16 ly + lx
  // this lane's B columns: patch offset of tap col (gathered), or the bias / padding column
  int ko[kWimgCT];
  float cb[kWimgCT];  // 1 for the bias column, 0 for padding columns, -1 for gathered columns
#pragma unroll
  for (int u = 0; u < kWimgCT; ++u) {
    const int col = (wave * kWimgCT + u) * 16 + j;
    const int ic = col / KK, rem = col - ic * KK, ky = rem / K, kx = rem - ky * K;
    ko[u] = col < Kt ? (ic * TI + ky) * TIP + kx : 0;
    cb[u] = col < Kt ? -1.0f : (col == Kt ? 1.0f : 0.0f);
  }
  const float* arow = dzl + (j < OC ? j : 0) * DZP;
  const float am = j < OC ? 1.0f : 0.0f;
  f4 acc[kWimgCT];
#pragma unroll
  for (int u = 0; u < kWimgCT; ++u) acc[u] = f4{0.f, 0.f, 0.f, 0.f};
  const size_t total_bytes = (size_t)a.n * a.x_stride;
  const int t0 = blockIdx.x * tpc, t1 = min(tiles, t0 + tpc);
  for (int t = t0; t < t1; ++t) {
    const int smp = t / tps, tt = t - smp * tps;
    const int ty = tt / tiles_x, tx = tt - ty * tiles_x;
    const int OH = a.OP / a.OW;
    const int x0 = tx * kImgTile * S, y0 = ty * kImgTile * S;
    __syncthreads();  // the previous tile's readers are done
    {
      const size_t sb = (size_t)smp * a.x_stride, left = total_bytes - sb;
      const PBuf ib{__builtin_amdgcn_make_buffer_rsrc((void*)(a.x_u8 + sb), (short)0,
                                                      (int)(left < 0xFFFFFFF0u ? left : 0xFFFFFFF0u), 0x00020000)};
      const int tot = a.IC * TI * DW;
      for (int e = tid; e < tot; e += 256) {
        const int ic = e / (TI * DW), rem = e - ic * (TI * DW), r = rem / DW, d = rem - r * DW;
        const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(ib.r, ic * plane + (y0 + r) * a.IW + x0 + 4 * d, 0, 0);
        *reinterpret_cast<unsigned*>(tile + (ic * TI + r) * TIP + 4 * d) = v;
      }
      const float* dz = a.dz + (size_t)smp * a.dz_stride;
      for (int e = tid; e < OC * 256; e += 256) {
        const int oc = e >> 8, px = e & 255, oy = ty * kImgTile + (px >> 4), ox = tx * kImgTile + (px & 15);
        const bool in = oy < OH && ox < a.OW;
        const float v = dz[in ? (size_t)oc * a.OP + oy * a.OW + ox : 0];
        dzl[oc * DZP + px] = in ? v : 0.0f;
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int st = 0; st < 64; ++st) {
      const int px = 4 * st + g, ly = px >> 4, lx = px & 15;
      const int po = S * ly * TIP + S * lx;
      const float av = arow[px] * am;
#pragma unroll
      for (int u = 0; u < kWimgCT; ++u) {
        const int raw = tile[ko[u] + po];
        const float xv = (float)raw * a.xscale;
        // columns >= Kt (bias, padding) exist only in the last tile of the last wave
        const float bv = u == kWimgCT - 1 ? (cb[u] < 0.0f ? xv : cb[u]) : xv;
        acc[u] = mfma16(av, bv, acc[u]);
      }
    }
  }
  float* out = a.part + (size_t)blockIdx.x * OC * (Kt + 1);
#pragma unroll
  for (int u = 0; u < kWimgCT; ++u) {
    const int col = (wave * kWimgCT + u) * 16 + j;
    if (col > Kt) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int oc = 4 * g + r;
      if (oc < OC) out[(size_t)oc * (Kt + 1) + col] = acc[u][r];
    }
  }
}

// ---- conv1's weight gradient with OC <= 8: two output columns per A row pair ------------------
// As k_conv_img2: A row oc + 8 dx is dZ[oc] at the odd (dx = 1) or even (dx = 0) output column of
// each column pair, the k dimension is the tile's 128 column pairs, and the B columns are the
// extended taps (ic, ky, kx'), kx' in [0, K + S), plus the bias column: D[oc + 8 dx][(ic, ky, kx')]
// sums dZ x input over the even (dx = 0) or odd (dx = 1) output columns, and
// dW[oc][ic, ky, kx] = D[oc][(ic, ky, kx)] + D[oc + 8][(ic, ky, kx + S)] (bias: both halves).
// 25 % fewer MFMAs than k_wgrad_img; the pixel sum is split into its even and odd halves, so the
// result differs from k_wgrad's in rounding only. The combine runs once per workgroup through LDS.
// The B operands are the raw byte values (exact in fp32) and the workgroup's tap sums are scaled by
// the image's scale (WgradArgs::xscale: 1 / 255, or 1 for a positional agent) once in the combine
// (round 5: one VALU fewer per MFMA; the bias column is not scaled).
constexpr int kWimg2CT = 9;  // column tiles per wave: 4 x 9 x 16 = 576 >= IC K (K + S) + 1 = 526
static size_t wimg2_lds_bytes(int IC, int K, int S, int OC) {
  const int TI = (kImgTile - 1) * S + K, TIP = (TI + 3) & ~3;
  const size_t patch = ((size_t)IC * TI * TIP + 15) & ~(size_t)15;
  const size_t stage = patch + (size_t)OC * 260 * 4, comb = (size_t)16 * 4 * kWimg2CT * 16 * 4;
  return stage > comb ? stage : comb;
}

// BX (create option conv1_mfma=bx3): the pixel sums as v_mfma_f32_16x16x32_bf16 — the B operands
// (raw bytes 0..255, and the bias column's 1) are exact bf16 numbers, so every fp32 product dZ.x is
// the exact sum of three: dZ's split-bf16 pieces (hi, mid, lo; split3_pair) times x. Three 16-cycle
// MFMAs per 32 pixel pairs instead of eight 32-cycle 16x16x4 f32 ones; lane group g's k slot e of
// step q is pixel pair 32 q + 4 e + g (the f32 loop's step 8 q + e).
template <int K, int S, bool BX = false>
__global__ __launch_bounds__(256, 3) void k_wgrad_img2(WgradArgs a, int tiles_x, int tps, int tiles, int tpc) {
  using G = ImgGeo<K, S>;
  constexpr int TI = G::TI, TIP = G::TIP, DW = TIP / 4, DZP = 260, KX = K + S, NC = 4 * kWimg2CT * 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int Kt = a.Kt, OC = a.OC, plane = a.IH * a.IW, Kx = a.IC * K * KX;
  const size_t patch = ((size_t)a.IC * TI * TIP + 15) & ~(size_t)15;
  unsigned char* tile = smem;
  float* dzl = reinterpret_cast<float*>(smem + patch);  // [OC][DZP]: pixel 16 ly + lx
  // B columns: extended tap col (gathered), the bias column (col == Kx) or padding
  int ko[kWimg2CT];
  float cb[kWimg2CT];  // 1 for the bias column, 0 for padding columns, -1 for gathered columns
#pragma unroll
  for (int u = 0; u < kWimg2CT; ++u) {
    const int col = (wave * kWimg2CT + u) * 16 + j;
    const int ic = col / (K * KX), rem = col - ic * (K * KX), ky = rem / KX, kxp = rem - ky * KX;
    ko[u] = col < Kx ? (ic * TI + ky) * TIP + kxp : 0;
    cb[u] = col < Kx ? -1.0f : (col == Kx ? 1.0f : 0.0f);
  }
  // A row j: channel j & 7 at the odd (j >= 8) or even column of each pair
  const int aoc = j & 7, adx = j >> 3;
  const float* arow = dzl + (aoc < OC ? aoc : 0) * DZP + adx;
  const float am = aoc < OC ? 1.0f : 0.0f;
  f4 acc[kWimg2CT];
#pragma unroll
  for (int u = 0; u < kWimg2CT; ++u) acc[u] = f4{0.f, 0.f, 0.f, 0.f};
  const size_t total_bytes = (size_t)a.n * a.x_stride;
  const int t0 = blockIdx.x * tpc, t1 = min(tiles, t0 + tpc);
  // staging (round 5): every load of a tile is issued at once into registers through buffer
  // descriptors (out-of-range offsets read 0), then stored, so no load waits on the previous one's
  // store (the loop form serialised ~27 load round trips per tile: 0.15 MFMA-pipe busy, 70 % of wave
  // cycles waiting). Prefetching the next tile during the MFMAs instead took 268 VGPRs (92 now).
  constexpr int NPE = (16 * TI * DW + 255) / 256, NZE = 8;  // launch condition: IC <= 16, OC <= 8
  const int tot = a.IC * TI * DW, OH = a.OP / a.OW;
  unsigned pv[NPE];
  float zv[NZE];
  auto sload = [&](int t) {
    const int smp = t / tps, tt = t - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    const int x0 = tx * kImgTile * S, y0 = ty * kImgTile * S;
    const size_t sb = (size_t)smp * a.x_stride, left = total_bytes - sb;
    const PBuf ib{__builtin_amdgcn_make_buffer_rsrc((void*)(a.x_u8 + sb), (short)0,
                                                    (int)(left < 0xFFFFFFF0u ? left : 0xFFFFFFF0u), 0x00020000)};
#pragma unroll
    for (int i = 0; i < NPE; ++i) {
      const int e = tid + 256 * i, ic = e / (TI * DW), rem = e - ic * (TI * DW), r = rem / DW, d = rem - r * DW;
      const uint32_t off = e < tot ? (uint32_t)(ic * plane + (y0 + r) * a.IW + x0 + 4 * d) : 0xFFFFFFF0u;
      pv[i] = __builtin_amdgcn_raw_buffer_load_b32(ib.r, off, 0, 0);
    }
    const PBuf zb{__builtin_amdgcn_make_buffer_rsrc((void*)(a.dz + (size_t)smp * a.dz_stride), (short)0,
                                                    (int)(a.dz_stride * 4), 0x00020000)};
#pragma unroll
    for (int i = 0; i < NZE; ++i) {
      const int e = tid + 256 * i, oc = e >> 8, px = e & 255, oy = ty * kImgTile + (px >> 4),
                ox = tx * kImgTile + (px & 15);
      const bool in = oc < OC && oy < OH && ox < a.OW;
      const uint32_t off = in ? (uint32_t)(oc * a.OP + oy * a.OW + ox) * 4u : 0x7ffffff0u;
      zv[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(zb.r, off, 0, 0));
    }
  };
  for (int t = t0; t < t1; ++t) {
    sload(t);
    __syncthreads();  // the previous tile's readers are done
#pragma unroll
    for (int i = 0; i < NPE; ++i) {
      const int e = tid + 256 * i, ic = e / (TI * DW), rem = e - ic * (TI * DW), r = rem / DW, d = rem - r * DW;
      if (e < tot) *reinterpret_cast<unsigned*>(tile + (ic * TI + r) * TIP + 4 * d) = pv[i];
    }
#pragma unroll
    for (int i = 0; i < NZE; ++i) {
      const int e = tid + 256 * i;
      if ((e >> 8) < OC) dzl[(e >> 8) * DZP + (e & 255)] = zv[i];
    }
    __syncthreads();
    if constexpr (BX) {
#pragma unroll 1
      for (int q = 0; q < 4; ++q) {
        u32x4 ah, amd, al;
#pragma unroll
        for (int w = 0; w < 4; ++w) {  // slots e = 2 w, 2 w + 1: rows 4 q + w, column pairs g, 4 + g
          const float* ar = arow + 16 * (4 * q + w) + 2 * g;
          unsigned h, md, l;
          split3_pair(ar[0] * am, ar[8] * am, h, md, l);
          ah[w] = h; amd[w] = md; al[w] = l;
        }
        const int po0 = S * 4 * q * TIP + 2 * S * g;
#pragma unroll
        for (int u = 0; u < kWimg2CT; ++u) {
          u32x4 b;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const int po = po0 + S * w * TIP;  // slot 2 w: column pair g; slot 2 w + 1: pair 4 + g
            float x0 = (float)tile[ko[u] + po], x1 = (float)tile[ko[u] + po + 8 * S];
            if (u >= kWimg2CT - 4 && cb[u] >= 0.0f) { x0 = cb[u]; x1 = cb[u]; }
            b[w] = pack_bf16_exact(x0, x1);
          }
          acc[u] = mfma16bx(al, b, acc[u]);
          acc[u] = mfma16bx(amd, b, acc[u]);
          acc[u] = mfma16bx(ah, b, acc[u]);
        }
      }
    } else {
#pragma unroll 4
    for (int st = 0; st < 32; ++st) {
      const int m = 4 * st + g, ly = m >> 3, lx2 = m & 7;  // column pair (2 lx2, 2 lx2 + 1) of row ly
      const int po = S * ly * TIP + 2 * S * lx2;
      const float av = arow[16 * ly + 2 * lx2] * am;
#pragma unroll
      for (int u = 0; u < kWimg2CT; ++u) {
        const int raw = tile[ko[u] + po];
        const float xv = (float)raw;  // the image's scale is applied once, in the combine below
        // the bias and padding columns lie in the last 4 tiles of the last wave (launch condition)
        const float bv = u >= kWimg2CT - 4 ? (cb[u] < 0.0f ? xv : cb[u]) : xv;
        acc[u] = mfma16(av, bv, acc[u]);
      }
    }
    }
  }
  // combine through LDS: D[16][NC] (row 4 g + r, column (wave 9 + u) 16 + j), then
  // dW[oc][(ic, ky, kx)] = D[oc][(ic, ky, kx)] + D[oc + 8][(ic, ky, kx + S)]
  __syncthreads();
  float* dl = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int u = 0; u < kWimg2CT; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) dl[(4 * g + r) * NC + (wave * kWimg2CT + u) * 16 + j] = acc[u][r];
  __syncthreads();
  float* out = a.part + (size_t)blockIdx.x * OC * (Kt + 1);
  for (int e = tid; e < OC * (Kt + 1); e += 256) {
    const int oc = e / (Kt + 1), k = e - oc * (Kt + 1);
    float v;
    if (k == Kt) {
      v = dl[oc * NC + Kx] + dl[(oc + 8) * NC + Kx];
    } else {
      const int ic = k / (K * K), rem = k - ic * (K * K), ky = rem / K, kx = rem - ky * K;
      const int c = (ic * K + ky) * KX + kx;
      v = (dl[oc * NC + c] + dl[(oc + 8) * NC + c + S]) * a.xscale;
    }
    out[e] = v;
  }
}

// ---- conv2's weight gradient from LDS-staged tiles (create option conv_wgrad=tiled, the default) ----
// k_wgrad gathers every B operand (an input value) from global memory, one buffer load per MFMA,
// which its counters show it waits on. Here a persistent workgroup walks output tiles of TY x TX
// pixels of one sample: the tile's dZ (OC x TY TX) and its input patch (IC x PH x PW, zero outside the
// plane) are staged in LDS, the next tile's loaded into registers while the current one computes.
// GEMM: rows = oc (A = dZ), columns = (ic, ky, kx) plus the bias column, k = the tile's pixels; wave w
// takes output rows RPW w .. + RPW - 1. For k-step kk a lane's B operand sits at its column's patch
// offset + the lane's pixel offset + an IMMEDIATE per kk, its A operand at one base + 4 kk: the k loop
// is ds_read_b32 + MFMA only. The bias column reads a block of ones. The workgroup keeps its sums in
// registers over all its tiles, adds its four waves in a fixed order through LDS and writes one
// partial per workgroup (k_wsum's layout); the sum order differs from k_wgrad's (tolerance tests).
constexpr int kWtTY = 8, kWtTX = 16;  // output tile (conv2: 45 x 45 -> 6 x 3 tiles, 88 % used)
// LDS layout (bank = dword address mod 32 for ds_read_b32, per 32-lane half = lane groups g = 0, 1):
// the patch rows are PW = 37 floats and each input channel's plane PPA = 713 floats, so column
// c = (ic, ky, kx) sits at a dword offset = c (mod 16) and a wave's 16 columns hit 16 distinct banks;
// lane group g takes the output columns kk % 4 + 8 (g & 1) + 4 (g >> 1), 16 input floats (16 banks) away
// for g = 1: the B reads are conflict-free. dZ rows are TQ + 1 floats (A reads: 2-way on half the banks).
template <int IC, int OC, int TY, int TX>
struct WtGeo {
  static constexpr int K = 5, S = 2, Kt = IC * K * K, NCT = (Kt + 1 + 15) / 16, NRT = OC / 16;
  static constexpr int PH = (TY - 1) * S + K, PWL = (TX - 1) * S + K, PW = 37, PPL = PH * PWL, TQ = TY * TX;
  static constexpr int PPA = ((PH * PW - 9 + 15) / 16) * 16 + 9;  // >= PH PW, = 9 (mod 16): ic planes step c by 25
  static constexpr int NXL = IC * PPL, NXP = IC * PPA, DZS = TQ + 1, NZ = OC * TQ, NZP = OC * DZS;
  static constexpr int RPW = TY / 4, KS = RPW * TX / 4;
  // the largest B offset a lane adds to its column base: wave rows, lane group and k-step parts
  static constexpr int BMAX = S * RPW * 3 * PW + 16 + 8 + S * (RPW - 1) * PW + S * 3;
  static constexpr int OB0 = NXP + NZP, ONES0 = OB0 + (((Kt - OB0) % 16) + 16) % 16;  // ones base = Kt (mod 16)
  static constexpr int LDS = ONES0 + BMAX + 1;
  static constexpr int RED = OC * NCT * 16;  // the wave reduction, aliased on the patch
  static_assert(PW >= PWL && PW % 16 == 5 && RED <= NXP, "layout");
};
template <int IC, int OC, int TY, int TX>
__global__ __launch_bounds__(256, 3) void k_wgrad_t(WgradArgs a, int tiles_x, int tps, int tiles) {
  using G = WtGeo<IC, OC, TY, TX>;
  constexpr int Kt = G::Kt, NCT = G::NCT, NRT = G::NRT, PW = G::PW, PWL = G::PWL, PPA = G::PPA, TQ = G::TQ,
                DZS = G::DZS, RPW = G::RPW, KS = G::KS, S = G::S;
  // staging runs over the padded layouts, so the LDS stores are linear in the thread index
  constexpr int NXP = G::NXP, NZP = G::NZP, NSX = (NXP + 255) / 256, NSZ = (NZP + 255) / 256;
  static_assert(OC % 16 == 0 && TY % 4 == 0 && TX == 16, "tile shape");
  __shared__ __attribute__((aligned(16))) float sm[G::LDS];
  float* xp = sm;                // [IC][PPA]: rows of PW
  float* dzt = sm + G::NXP;      // [OC][DZS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  for (int i = G::OB0 + tid; i < G::LDS; i += 256) sm[i] = 1.0f;  // the bias column's B operands
  // column bases: (ic, ky, kx) -> ic PPA + ky PW + kx; the bias column -> the ones; padding -> any
  // in-patch offset = c (mod 16)
  int cb[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int c = 16 * ct + j, ic = c / 25, r = c - 25 * ic, ky = r / 5, kx = r - 5 * ky;
    cb[ct] = c < Kt ? ic * PPA + ky * PW + kx : (c == Kt ? G::ONES0 : (c & 15));
  }
  const int bb = S * RPW * wave * PW + 16 * (g & 1) + 8 * (g >> 1);  // + S (kk / 4) PW + S (kk % 4)
  const int ab = j * DZS + RPW * TX * wave + 8 * (g & 1) + 4 * (g >> 1);  // + 16 rt DZS + TX (kk / 4) + kk % 4
  const long plane = (long)a.IH * a.IW;
  const int OH = a.OP / a.OW;
  float sx[NSX], sz[NSZ];
  auto sload = [&](int tile) {
    int tidv = tid;  // opaque: the per-element offsets are recomputed per tile, not hoisted (registers)
    asm volatile("" : "+v"(tidv));
    const int smp = tile / tps, tt = tile - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    const PBuf xb{__builtin_amdgcn_make_buffer_rsrc((void*)(a.x_f + (size_t)smp * a.x_stride), (short)0,
                                                    (int)(a.x_stride * 4), 0x00020000)};
    const PBuf zb{__builtin_amdgcn_make_buffer_rsrc((void*)(a.dz + (size_t)smp * a.dz_stride), (short)0,
                                                    (int)(a.dz_stride * 4), 0x00020000)};
    const int iy0 = S * TY * ty, ix0 = S * TX * tx, oy0 = TY * ty, ox0 = TX * tx;
#pragma unroll
    for (int i = 0; i < NSX; ++i) {
      const int e = tidv + 256 * i, ic = e / PPA, rem = e - ic * PPA, r = rem / PW, c = rem - r * PW;
      const int iy = iy0 + r, ix = ix0 + c;
      const bool in = e < NXP && r < G::PH && c < PWL && iy < a.IH && ix < a.IW;
      const uint32_t off = in ? (uint32_t)(ic * plane + iy * a.IW + ix) * 4u : 0x7ffffff0u;
      sx[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xb.r, off, 0, 0));
    }
#pragma unroll
    for (int i = 0; i < NSZ; ++i) {
      const int e = tidv + 256 * i, oc = e / DZS, q = e - oc * DZS, oy = oy0 + q / TX, ox = ox0 + q % TX;
      const bool in = e < NZP && q < TQ && oy < OH && ox < a.OW;
      const uint32_t off = in ? (uint32_t)(oc * a.OP + oy * a.OW + ox) * 4u : 0x7ffffff0u;
      sz[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(zb.r, off, 0, 0));
    }
  };
  f4 acc[NRT][NCT];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[rt][ct] = f4{0.f, 0.f, 0.f, 0.f};
  if ((int)blockIdx.x < tiles) sload(blockIdx.x);
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < NSX; ++i)
      if (tid + 256 * i < NXP) xp[tid + 256 * i] = sx[i];
#pragma unroll
    for (int i = 0; i < NSZ; ++i)
      if (tid + 256 * i < NZP) dzt[tid + 256 * i] = sz[i];
    __syncthreads();
    if (tile + (int)gridDim.x < tiles) sload(tile + gridDim.x);
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int boff = S * (kk / 4) * PW + S * (kk % 4), aoff = TX * (kk / 4) + kk % 4;
      float av[NRT];
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) av[rt] = dzt[ab + 16 * rt * DZS + aoff];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const float bv = xp[cb[ct] + bb + boff];
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) acc[rt][ct] = mfma16(av[rt], bv, acc[rt][ct]);
      }
    }
    __syncthreads();  // every wave is done with the tile before the next one is stored
  }
  // the four waves' sums in wave order through LDS (aliasing the patch), then one partial per workgroup
  float* red = sm;  // [OC][NCT * 16]
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* p = red + (16 * rt + 4 * g + r) * (NCT * 16) + 16 * ct + j;
            *p = w ? *p + acc[rt][ct][r] : acc[rt][ct][r];
          }
    }
    __syncthreads();
  }
  float* out = a.part + (size_t)blockIdx.x * OC * (Kt + 1);
  for (int i = tid; i < OC * (Kt + 1); i += 256) {
    const int oc = i / (Kt + 1), c = i - oc * (Kt + 1);
    out[i] = red[oc * (NCT * 16) + c];
  }
}

// ---- conv3's weight gradient (IC 16, OC 32): k_wgrad_t with the COLUMNS split over the waves ---------
// Same staging and GEMM as k_wgrad_t, but 401 columns x 32 rows do not fit one wave's registers: wave w
// takes column tiles w, w + 4, ... over all TQ pixels of the tile (no cross-wave reduction), and the
// tile is TY x TX = 8 x 8 (conv3's 21 x 21 output: 3 x 3 tiles, 77 % used). Patch rows PW = 5 (mod 16)
// and planes PPA = 9 (mod 16) floats as in k_wgrad_t; dZ rows TQ + 2 floats (A reads: lane groups 0 and
// 1 on even / odd banks). Each lane group g takes pixel 4 kk + g of k-step kk.
constexpr int kWt2TY = 8, kWt2TX = 8;
template <int IC, int OC, int TY, int TX>
struct Wt2Geo {
  static constexpr int K = 5, S = 2, Kt = IC * K * K, NCT = (Kt + 1 + 15) / 16, NCW = (NCT + 3) / 4, NRT = OC / 16;
  static constexpr int PH = (TY - 1) * S + K, PWL = (TX - 1) * S + K, PW = ((PWL - 5 + 15) / 16) * 16 + 5;
  static constexpr int PPA = ((PH * PW - 9 + 15) / 16) * 16 + 9, TQ = TY * TX, DZS = TQ + 2, KS = TQ / 4;
  static constexpr int NXP = IC * PPA, NZP = OC * DZS;
  static constexpr int BMAX = S * (KS / (TX / 4) - 1) * PW + S * 4 * (TX / 4 - 1) + S * 3;
  static constexpr int OB0 = NXP + NZP, ONES0 = OB0 + (((Kt - OB0) % 16) + 16) % 16;
  static constexpr int LDS = ONES0 + BMAX + 1;
  static_assert(PW >= PWL && PPA >= PH * PW && TX % 4 == 0 && OC % 16 == 0, "layout");
};
template <int IC, int OC, int TY, int TX>
__global__ __launch_bounds__(256, 4) void k_wgrad_t2(WgradArgs a, int tiles_x, int tps, int tiles) {
  using G = Wt2Geo<IC, OC, TY, TX>;
  constexpr int Kt = G::Kt, NCT = G::NCT, NCW = G::NCW, NRT = G::NRT, PW = G::PW, PWL = G::PWL, PPA = G::PPA,
                TQ = G::TQ, DZS = G::DZS, KS = G::KS, S = G::S, NXP = G::NXP, NZP = G::NZP;
  constexpr int NSX = (NXP + 255) / 256, NSZ = (NZP + 255) / 256;
  __shared__ __attribute__((aligned(16))) float sm[G::LDS];
  float* xp = sm;            // [IC][PPA]: rows of PW
  float* dzt = sm + NXP;     // [OC][DZS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  for (int i = G::OB0 + tid; i < G::LDS; i += 256) sm[i] = 1.0f;  // the bias column's B operands
  int cb[NCW];
#pragma unroll
  for (int i = 0; i < NCW; ++i) {
    const int c = 16 * (wave + 4 * i) + j, ic = c / 25, r = c - 25 * ic, ky = r / 5, kx = r - 5 * ky;
    cb[i] = c < Kt ? ic * PPA + ky * PW + kx : (c == Kt ? G::ONES0 : (c & 15));
  }
  const int bb = S * g, ab = j * DZS + g;  // B: + S (kk / (TX / 4)) PW + 4 S (kk % (TX / 4)); A: + 16 rt DZS + 4 kk
  const long plane = (long)a.IH * a.IW;
  const int OH = a.OP / a.OW;
  float sx[NSX], sz[NSZ];
  auto sload = [&](int tile) {
    int tidv = tid;  // opaque: the per-element offsets are recomputed per tile, not hoisted (registers)
    asm volatile("" : "+v"(tidv));
    const int smp = tile / tps, tt = tile - smp * tps, ty = tt / tiles_x, tx = tt - ty * tiles_x;
    const PBuf xb{__builtin_amdgcn_make_buffer_rsrc((void*)(a.x_f + (size_t)smp * a.x_stride), (short)0,
                                                    (int)(a.x_stride * 4), 0x00020000)};
    const PBuf zb{__builtin_amdgcn_make_buffer_rsrc((void*)(a.dz + (size_t)smp * a.dz_stride), (short)0,
                                                    (int)(a.dz_stride * 4), 0x00020000)};
    const int iy0 = S * TY * ty, ix0 = S * TX * tx, oy0 = TY * ty, ox0 = TX * tx;
#pragma unroll
    for (int i = 0; i < NSX; ++i) {
      const int e = tidv + 256 * i, ic = e / PPA, rem = e - ic * PPA, r = rem / PW, c = rem - r * PW;
      const int iy = iy0 + r, ix = ix0 + c;
      const bool in = e < NXP && r < G::PH && c < PWL && iy < a.IH && ix < a.IW;
      const uint32_t off = in ? (uint32_t)(ic * plane + iy * a.IW + ix) * 4u : 0x7ffffff0u;
      sx[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xb.r, off, 0, 0));
    }
#pragma unroll
    for (int i = 0; i < NSZ; ++i) {
      const int e = tidv + 256 * i, oc = e / DZS, q = e - oc * DZS, oy = oy0 + q / TX, ox = ox0 + q % TX;
      const bool in = e < NZP && q < TQ && oy < OH && ox < a.OW;
      const uint32_t off = in ? (uint32_t)(oc * a.OP + oy * a.OW + ox) * 4u : 0x7ffffff0u;
      sz[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(zb.r, off, 0, 0));
    }
  };
  f4 acc[NRT][NCW];
#pragma unroll
  for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
    for (int i = 0; i < NCW; ++i) acc[rt][i] = f4{0.f, 0.f, 0.f, 0.f};
  if ((int)blockIdx.x < tiles) sload(blockIdx.x);
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < NSX; ++i)
      if (tid + 256 * i < NXP) xp[tid + 256 * i] = sx[i];
#pragma unroll
    for (int i = 0; i < NSZ; ++i)
      if (tid + 256 * i < NZP) dzt[tid + 256 * i] = sz[i];
    __syncthreads();
    if (tile + (int)gridDim.x < tiles) sload(tile + gridDim.x);
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int boff = S * (kk / (TX / 4)) * PW + 4 * S * (kk % (TX / 4));
      float av[NRT];
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) av[rt] = dzt[ab + 16 * rt * DZS + 4 * kk];
#pragma unroll
      for (int i = 0; i < NCW; ++i) {
        if (wave + 4 * i >= NCT) continue;  // wave-uniform
        const float bv = xp[cb[i] + bb + boff];
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) acc[rt][i] = mfma16(av[rt], bv, acc[rt][i]);
      }
    }
    __syncthreads();  // every wave is done with the tile before the next one is stored
  }
  float* out = a.part + (size_t)blockIdx.x * OC * (Kt + 1);
#pragma unroll
  for (int i = 0; i < NCW; ++i) {
    const int c = 16 * (wave + 4 * i) + j;
    if (c > Kt) continue;
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)(16 * rt + 4 * g + r) * (Kt + 1) + c] = acc[rt][i][r];
  }
}

// G[w + oc*wstride + k] / G[b + oc] = sum over chunks (wstride = Kt, or more where the filters hold
// channels the gathered columns do not cover: a positional agent's conv1). Level 1 (k_wsum1) adds groups of kSumGroup
// consecutive chunks in parallel (blockIdx.y = group), level 2 (k_wsum) adds the group sums in order:
// a fixed order, so the result is deterministic.
constexpr int kSumGroup = 32;

__global__ void k_wsum1(const float* __restrict__ part, int chunks, long per, float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= per) return;
  const int c0 = blockIdx.y * kSumGroup, c1 = c0 + kSumGroup < chunks ? c0 + kSumGroup : chunks;
  float acc = 0.f;
  for (int c = c0; c < c1; ++c) acc += part[(long)c * per + i];
  out[(long)blockIdx.y * per + i] = acc;
}

__global__ void k_wsum(const float* __restrict__ part, int chunks, int OC, int Kt, int wstride,
                       float* __restrict__ Gw, float* __restrict__ Gb, int accum) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)OC * (Kt + 1);
  if (i >= per) return;
  float acc = 0.f;
  for (int c = 0; c < chunks; ++c) acc += part[(long)c * per + i];
  const int oc = (int)(i / (Kt + 1)), k = (int)(i - (long)oc * (Kt + 1));
  float* o = k < Kt ? Gw + (long)oc * wstride + k : Gb + oc;
  *o = accum ? *o + acc : acc;  // accum: a later sample group of launch_wgrad's split
}

}  // namespace

int launch_dgrad(const DgradArgs& a, hipStream_t s, bool staged, bool quad) {
  if (staged && quad && a.K == 5 && a.S == 2 && a.IC == 16 && a.OC == 32 && a.w_ic == a.IC) {
    const int tiles_x = ((a.IW + 1) / 2 + kDq2T - 1) / kDq2T, tps = tiles_x * (((a.IH + 1) / 2 + kDq2T - 1) / kDq2T);
    const long tiles = (long)a.n * tps;
    const size_t lds = dq2_lds_bytes(a.OC);
    static const bool attr = hipFuncSetAttribute((const void*)k_dgrad_q2<16, 32>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
    if (attr && tiles < (1L << 31) && a.dz_stride < (1L << 29) && a.x_stride < (1L << 29) && a.dx_stride < (1L << 29)) {
      const int grid = (int)std::min<long>(tiles, 256L * 2);  // two workgroups per CU (LDS)
      hipLaunchKernelGGL((k_dgrad_q2<16, 32>), dim3(grid), dim3(256), lds, s, a, tiles_x, tps, (int)tiles);
      return 0;
    }
  }
  if (staged && quad && a.K == 5 && a.S == 2 && a.IC == 8 && a.OC == 16 && a.w_ic == a.IC && a.IW % 2 == 0) {
    const int tiles_x = ((a.IW + 1) / 2 + kDqT - 1) / kDqT, tps = tiles_x * (((a.IH + 1) / 2 + 4 * kDqU - 1) / (4 * kDqU));
    const long tiles = (long)a.n * tps;
    if (tiles >= (1L << 31) || a.dz_stride >= (1L << 29) || a.x_stride >= (1L << 29) || a.dx_stride >= (1L << 29))
      return -1;
    // one round of resident workgroups (kDqU = 2: three per CU; 4: two): a larger grid would run a
    // second, partial round
    const int grid = (int)std::min<long>(tiles, 256L * (kDqU == 2 ? 3 : 2));
    hipLaunchKernelGGL((k_dgrad_q<8, 16>), dim3(grid), dim3(256), 0, s, a, tiles_x, tps, (int)tiles);
    return 0;
  }
  if (staged && a.K == 5 && a.S == 2 && a.IC <= 16 && a.OC <= 16 && a.w_ic == a.IC &&
      ds2_lds_bytes(a.IC, a.OC) <= 64 * 1024) {
    const int tiles_x = (a.IW + kDs2Tile - 1) / kDs2Tile, tps = tiles_x * ((a.IH + kDs2Tile - 1) / kDs2Tile);
    hipLaunchKernelGGL(k_dgrad_s2, dim3(a.n * tps), dim3(256), ds2_lds_bytes(a.IC, a.OC), s, a, tiles_x, tps);
    return 0;
  }
  const int nj = (a.K + a.S - 1) / a.S;
  if ((long)a.OC * nj * nj > kMaxDTab) return -1;
  const int H2 = (a.IH + a.S - 1) / a.S, W2 = (a.IW + a.S - 1) / a.S;
  const long Q = (long)a.n * H2 * W2;
  const int np = Q >= 16L * 4 * 1024 ? 4 : 1;
  const unsigned gx = (unsigned)((Q + 64L * np - 1) / (64L * np));
  const unsigned gz = (unsigned)(a.S * a.S);
  if (a.IC >= 64) {
    if (np == 4) hipLaunchKernelGGL((k_dgrad<4, 4>), dim3(gx, (a.IC + 63) / 64, gz), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_dgrad<4, 1>), dim3(gx, (a.IC + 63) / 64, gz), dim3(256), 0, s, a);
  } else if (a.IC >= 32) {
    if (np == 4) hipLaunchKernelGGL((k_dgrad<2, 4>), dim3(gx, (a.IC + 31) / 32, gz), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_dgrad<2, 1>), dim3(gx, (a.IC + 31) / 32, gz), dim3(256), 0, s, a);
  } else {
    if (np == 4) hipLaunchKernelGGL((k_dgrad<1, 4>), dim3(gx, (a.IC + 15) / 16, gz), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_dgrad<1, 1>), dim3(gx, (a.IC + 15) / 16, gz), dim3(256), 0, s, a);
  }
  return 0;
}

// A 3 x 3 stride-1 layer on a tiny plane (dgrad_col_layer) as a dense GEMM + col2im: wt [IC K K][OC],
// zbias [IC K K] zeros and dcol [n][IC K K][OH OW] are the caller's scratch (carla_train_init)
int launch_dgrad_col(const DgradArgs& a, float* wt, const float* zbias, float* dcol, hipStream_t s) {
  const int kt = a.IC * a.K * a.K, OP = a.OH * a.OW;
  hipLaunchKernelGGL(k_wtrans, dim3((unsigned)(((long)kt * a.OC + 255) / 256)), dim3(256), 0, s, a.W, a.OC, kt, wt);
  ConvArgs ca{a.dz,  nullptr, a.dz_stride, a.OC, a.OH, a.OW, wt, zbias, dcol, (long)kt * OP, kt, a.OH, a.OW, 1, 1, 0,
              a.n, nullptr, 0};
  const int bad = launch_conv(ca, s, 0);
  const long tot = (long)a.n * a.x_stride;
  const dim3 cg((unsigned)((tot + 255) / 256));
  if (a.S == 1)
    hipLaunchKernelGGL((k_col2im<3, 1>), cg, dim3(256), 0, s, dcol, a.x, a.x_stride, a.dx, a.dx_stride, a.IC, a.IH,
                       a.IW, a.OH, a.OW, a.n, 0);
  else
    hipLaunchKernelGGL((k_col2im<3, 2>), cg, dim3(256), 0, s, dcol, a.x, a.x_stride, a.dx, a.dx_stride, a.IC, a.IH,
                       a.IW, a.OH, a.OW, a.n, 0);
  return bad;
}

constexpr int kWgradNKT = 2;  // a wave: 32 gathered columns; a workgroup: 128

WgradPlan plan_wgrad(int OC, int Kt, long Q) {
  WgradPlan p;
  p.not_ = OC >= 64 ? 4 : (OC >= 32 ? 2 : 1);
  p.ocg = (OC + 16 * p.not_ - 1) / (16 * p.not_);
  p.kg = (Kt + 1 + 64 * kWgradNKT - 1) / (64 * kWgradNKT);
  long chunks = (8192 + (long)p.ocg * p.kg - 1) / ((long)p.ocg * p.kg);
  chunks = chunks < 1 ? 1 : (chunks > 4096 ? 4096 : chunks);
  const long cap = (32L << 20) / ((long)OC * (Kt + 1));  // partials <= 32 M floats
  if (chunks > cap) chunks = cap < 1 ? 1 : cap;
  // at least 64 pixels / rows per chunk: the Linear layers (2 048 rows) then need <= 32 chunks and
  // one k_wsum pass instead of k_wsum1 + k_wsum
  const long maxc = (Q + 63) / 64;
  if (chunks > maxc) chunks = maxc < 1 ? 1 : maxc;
  p.qchunk = ((Q + chunks - 1) / chunks + 3) / 4 * 4;
  p.chunks = (int)((Q + p.qchunk - 1) / p.qchunk);
  const int groups = (p.chunks + kSumGroup - 1) / kSumGroup;
  p.part_floats = (size_t)(p.chunks + (p.chunks > kSumGroup ? groups : 0)) * OC * (Kt + 1);
  return p;
}

// the chunk sums that end every weight-gradient launch: a.part holds `chunks` partials [OC][Kt + 1]; more
// than kSumGroup of them go through one level of group sums, written after the partials (sized by
// plan_wgrad and the launchers' capacity checks). accum: add to Gw / Gb instead of storing
static void launch_wsum(const WgradArgs& a, int chunks, float* Gw, float* Gb, int accum, hipStream_t s) {
  const long per = (long)a.OC * (a.Kt + 1);
  const unsigned gb = (unsigned)((per + 255) / 256);
  const int ws = a.wstride ? a.wstride : a.Kt;
  if (chunks > kSumGroup) {
    const int groups = (chunks + kSumGroup - 1) / kSumGroup;
    float* lvl = a.part + (size_t)chunks * per;
    hipLaunchKernelGGL(k_wsum1, dim3(gb, groups), dim3(256), 0, s, a.part, chunks, per, lvl);
    hipLaunchKernelGGL(k_wsum, dim3(gb), dim3(256), 0, s, lvl, groups, a.OC, a.Kt, ws, Gw, Gb, accum);
  } else {
    hipLaunchKernelGGL(k_wsum, dim3(gb), dim3(256), 0, s, a.part, chunks, a.OC, a.Kt, ws, Gw, Gb, accum);
  }
}

// the generic gather kernel k_wgrad (+ its chunk sums). Its fp32 gathers use 32-bit buffer offsets
// over the whole input, so an input of >= 0x70000000 bytes runs as consecutive sample groups below
// that size, each group's sums added to the previous ones' (accum)
static int launch_wgrad_generic(WgradArgs a, float* Gw, float* Gb, float* part, size_t part_cap, hipStream_t s,
                                int accum = 0) {
  const long lim = a.group_bytes > 0 && a.group_bytes < (long)kWgradFar ? a.group_bytes : (long)kWgradFar;
  if (!a.x_u8 && (long)a.n * a.x_stride * 4 >= lim) {
    const long ns = (lim / 4 - 1) / (a.x_stride > 0 ? a.x_stride : 1);
    if (ns < 1) return -1;
    for (long s0 = 0; s0 < a.n; s0 += ns) {
      WgradArgs b = a;
      b.n = (int)std::min<long>(ns, a.n - s0);
      b.x_f = a.x_f + s0 * a.x_stride;
      b.dz = a.dz + s0 * a.dz_stride;
      if (launch_wgrad_generic(b, Gw, Gb, part, part_cap, s, accum || s0 > 0)) return -1;
    }
    return 0;
  }
  const WgradPlan p = plan_wgrad(a.OC, a.Kt, (long)a.n * a.OP);
  if (p.part_floats > part_cap) return -1;
  a.qchunk = p.qchunk;
  a.part = part;
  const dim3 grid(p.chunks, p.ocg, p.kg);
  if (a.x_u8) {
    if (p.not_ == 4) hipLaunchKernelGGL((k_wgrad<4, kWgradNKT, true>), grid, dim3(256), 0, s, a);
    else if (p.not_ == 2) hipLaunchKernelGGL((k_wgrad<2, kWgradNKT, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_wgrad<1, kWgradNKT, true>), grid, dim3(256), 0, s, a);
  } else {
    if (p.not_ == 4) hipLaunchKernelGGL((k_wgrad<4, kWgradNKT, false>), grid, dim3(256), 0, s, a);
    else if (p.not_ == 2) hipLaunchKernelGGL((k_wgrad<2, kWgradNKT, false>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_wgrad<1, kWgradNKT, false>), grid, dim3(256), 0, s, a);
  }
  launch_wsum(a, p.chunks, Gw, Gb, accum, s);
  return 0;
}

int launch_wgrad(WgradArgs a, float* Gw, float* Gb, float* part, size_t part_cap, hipStream_t s, bool img, bool bx,
                 bool tiled) {
  if (a.Kt > kMaxKTab || a.OP > kMaxPTab) return -1;
  const long per = (long)a.OC * (a.Kt + 1);
  const int OH = a.OP / a.OW;
  const bool c2 = a.IC == 8 && a.OC == 16, c3 = a.IC == 16 && a.OC == 32;
  if (img && tiled && a.x_f && a.K == 5 && a.S == 2 && (c2 || c3) && a.dz_stride < (1L << 29) && a.x_stride < (1L << 29)) {
    const int TY = c2 ? kWtTY : kWt2TY, TX = c2 ? kWtTX : kWt2TX;
    const int tiles_x = (a.OW + TX - 1) / TX, tps = tiles_x * ((OH + TY - 1) / TY);
    const long tiles = (long)a.n * tps;
    // one round of resident workgroups: k_wgrad_t three per CU (137 VGPRs), k_wgrad_t2 four (112)
    const int chunks = (int)std::min<long>(tiles, c2 ? 768 : 1024);
    const int groups = (chunks + kSumGroup - 1) / kSumGroup;
    if (tiles < (1L << 31) && (size_t)(chunks + (chunks > kSumGroup ? groups : 0)) * per <= part_cap) {
      a.part = part;
      if (c2)
        hipLaunchKernelGGL((k_wgrad_t<8, 16, kWtTY, kWtTX>), dim3(chunks), dim3(256), 0, s, a, tiles_x, tps, (int)tiles);
      else
        hipLaunchKernelGGL((k_wgrad_t2<16, 32, kWt2TY, kWt2TX>), dim3(chunks), dim3(256), 0, s, a, tiles_x, tps,
                           (int)tiles);
      launch_wsum(a, chunks, Gw, Gb, 0, s);
      return 0;
    }
  }
  if (img && a.x_u8 && ((uintptr_t)a.x_u8 & 3) == 0 && a.K == 5 && a.S == 2 && a.OC <= 8 &&
      a.IC * a.K * (a.K + a.S) + 1 <= 4 * kWimg2CT * 16 && a.IC * a.K * (a.K + a.S) >= (4 * kWimg2CT - 4) * 16 &&
      a.IW % 4 == 0 && a.x_stride % 4 == 0 &&
      wimg2_lds_bytes(a.IC, a.K, a.S, a.OC) <= 64 * 1024) {
    const int tiles_x = (a.OW + kImgTile - 1) / kImgTile, tiles_y = (OH + kImgTile - 1) / kImgTile;
    const int tiles = a.n * tiles_x * tiles_y;
    int chunks = std::min(tiles, 768);  // three workgroups per CU (168 VGPRs): one round
    const int tpc = (tiles + chunks - 1) / chunks;
    chunks = (tiles + tpc - 1) / tpc;
    const int groups = (chunks + kSumGroup - 1) / kSumGroup;
    if ((size_t)(chunks + (chunks > kSumGroup ? groups : 0)) * per <= part_cap) {
      a.part = part;
      if (bx)
        hipLaunchKernelGGL((k_wgrad_img2<5, 2, true>), dim3(chunks), dim3(256), wimg2_lds_bytes(a.IC, a.K, a.S, a.OC),
                           s, a, tiles_x, tiles_x * tiles_y, tiles, tpc);
      else
        hipLaunchKernelGGL((k_wgrad_img2<5, 2, false>), dim3(chunks), dim3(256), wimg2_lds_bytes(a.IC, a.K, a.S, a.OC),
                           s, a, tiles_x, tiles_x * tiles_y, tiles, tpc);
      launch_wsum(a, chunks, Gw, Gb, 0, s);
      return 0;
    }
  }
  if (img && a.x_u8 && ((uintptr_t)a.x_u8 & 3) == 0 && a.K == 5 && a.S == 2 && a.OC <= 16 &&
      a.Kt + 1 <= 4 * kWimgCT * 16 &&
      a.Kt >= (4 * kWimgCT - 1) * 16 && a.IW % 4 == 0 &&
      a.x_stride % 4 == 0 && wimg_lds_bytes(a.IC, a.K, a.S, a.OC) <= 64 * 1024) {
    const int tiles_x = (a.OW + kImgTile - 1) / kImgTile, tiles_y = (OH + kImgTile - 1) / kImgTile;
    const int tiles = a.n * tiles_x * tiles_y;
    int chunks = std::min(tiles, 1024);
    const int tpc = (tiles + chunks - 1) / chunks;
    chunks = (tiles + tpc - 1) / tpc;
    const int groups = (chunks + kSumGroup - 1) / kSumGroup;
    if ((size_t)(chunks + (chunks > kSumGroup ? groups : 0)) * per <= part_cap) {
      a.part = part;
      hipLaunchKernelGGL((k_wgrad_img<5, 2>), dim3(chunks), dim3(256), wimg_lds_bytes(a.IC, a.K, a.S, a.OC), s, a,
                         tiles_x, tiles_x * tiles_y, tiles, tpc);
      launch_wsum(a, chunks, Gw, Gb, 0, s);
      return 0;
    }
  }
  return launch_wgrad_generic(a, Gw, Gb, part, part_cap, s);
}
