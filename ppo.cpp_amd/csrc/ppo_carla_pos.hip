// ppo_carla_pos.hip — use_positional_encoding (include/ppo_carla.h; reference carla_model.h:38-42, :222-236).
//
// The reference appends two planes to the bev before cnn.0: plane C holds linspace(-1, 1, IH)[row], plane
// C + 1 holds linspace(-1, 1, IW)[col] (meshgrid "ij"). They are the same for every sample, plane C is
// constant along x and plane C + 1 along y, and the convolution has no padding, so their part of conv1's
// pre-activation is separable and their weight gradient needs only row and column sums of dZ1:
//
//   Zpos[oc, oy, ox] = rowb[oc, oy] + colb[oc, ox]
//   rowb[oc, oy] = sum_ky linH[S oy + ky] * sum_kx W[oc, C,     ky, kx]
//   colb[oc, ox] = sum_kx linW[S ox + kx] * sum_ky W[oc, C + 1, ky, kx]
//
//   R[oc, oy] = sum_{n, ox} dZ1[n, oc, oy, ox]      Q[oc, ox] = sum_{n, oy} dZ1[n, oc, oy, ox]
//   dW[oc, C,     ky, kx] = sum_oy linH[S oy + ky] * R[oc, oy]      (the same for every kx)
//   dW[oc, C + 1, ky, kx] = sum_ox linW[S ox + kx] * Q[oc, ox]      (the same for every ky)
//
// So no [n, C + 2, H, W] input exists anywhere: the conv1 kernels read the image channels of the wider
// filter (ConvArgs::wstride) and add rowb + colb with the bias; the backward adds one streaming pass
// over dZ1 (k_pos_rq) and one small finish (k_pos_wfin). Every sum has a fixed order and there are no
// floating-point atomics: two updates on the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "ppo_carla_units.hpp"

namespace {

// one thread per table entry: e < OC * (OH + OW)
__global__ __launch_bounds__(256) void k_pos_bias(const float* __restrict__ W, int OC, int ICt, int C, int K, int S,
                                                  int IH, int IW, int OH, int OW, float* __restrict__ rowb,
                                                  float* __restrict__ colb) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= OC * (OH + OW)) return;
  const int oc = e / (OH + OW), r = e - oc * (OH + OW);
  const float* w = W + ((long)oc * ICt + C) * K * K;  // plane C; plane C + 1 follows
  float acc = 0.f;
  if (r < OH) {
    for (int ky = 0; ky < K; ++ky) {
      float sw = 0.f;
      for (int kx = 0; kx < K; ++kx) sw += w[ky * K + kx];
      acc = fmaf(pos_lin(S * r + ky, IH), sw, acc);
    }
    rowb[oc * OH + r] = acc;
  } else {
    const int ox = r - OH;
    w += K * K;
    for (int kx = 0; kx < K; ++kx) {
      float sw = 0.f;
      for (int ky = 0; ky < K; ++ky) sw += w[ky * K + kx];
      acc = fmaf(pos_lin(S * ox + kx, IW), sw, acc);
    }
    colb[oc * OW + ox] = acc;
  }
}

__device__ __forceinline__ float pos_wave_sum(float v) {  // every lane gets the same fixed-order total
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Row and column sums of dz over the samples [kPosSPC c, kPosSPC (c + 1)) of channel oc = blockIdx.y.
// Wave w streams rows w, w + 4, ... of each plane, two rows in flight; lane l owns columns l + 64 q. A
// column sum stays in the lane's register over all rows and samples; a row sum is one fixed xor tree
// over the wave, added by lane 0 to the row's LDS cell (a row belongs to one wave). The four waves'
// column sums are added in wave order at the end. partR [chunks][OC][OH], partQ [chunks][OC][OW].
__global__ __launch_bounds__(256) void k_pos_rq(const float* __restrict__ dz, long dz_stride, int n, int OH, int OW,
                                                float* __restrict__ partR, float* __restrict__ partQ) {
  __shared__ float rows[kPosMaxOH];
  __shared__ float cols[4][kPosMaxOW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int oc = blockIdx.y, OC = gridDim.y;
  const int s0 = blockIdx.x * kPosSPC, s1 = min(n, s0 + kPosSPC);
  for (int oy = tid; oy < OH; oy += 256) rows[oy] = 0.f;
  __syncthreads();
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  for (int smp = s0; smp < s1; ++smp) {
    const float* pl = dz + (long)smp * dz_stride + (long)oc * OH * OW;
    for (int oy = wave; oy < OH; oy += 8) {
      const bool two = oy + 4 < OH;
      float v[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ox = lane + 64 * q;
          const bool ok = ox < OW && (h == 0 || two);
          v[h][q] = ok ? pl[(long)(oy + 4 * h) * OW + ox] : 0.f;
        }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int q = 0; q < 4; ++q) cs[q] += v[h][q];
        const float r = pos_wave_sum((v[h][0] + v[h][1]) + (v[h][2] + v[h][3]));
        if (lane == 0 && (h == 0 || two)) rows[oy + 4 * h] += r;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) cols[wave][lane + 64 * q] = cs[q];
  __syncthreads();
  const long base = (long)blockIdx.x * OC + oc;
  for (int oy = tid; oy < OH; oy += 256) partR[base * OH + oy] = rows[oy];
  if (tid < OW) partQ[base * OW + tid] = (cols[0][tid] + cols[1][tid]) + (cols[2][tid] + cols[3][tid]);
}

// The chunk sums of channel oc = blockIdx.x (R, Q into LDS): each of the block's four 256-thread groups adds
// one contiguous quarter of the chunks in chunk order, the quarters are added in a fixed tree. Then
// thread (which, k) of the first 2 K: the dot product with the shifted grid, written to the K filter
// entries that share it.
constexpr int kPosFinGroups = 4;
__global__ __launch_bounds__(256 * kPosFinGroups) void k_pos_wfin(const float* __restrict__ partR,
                                                                  const float* __restrict__ partQ, int chunks, int OH,
                                                                  int OW, int K, int S, int IH, int IW,
                                                                  float* __restrict__ dw, long dw_stride) {
  __shared__ float red[kPosFinGroups][kPosMaxOH + kPosMaxOW];
  __shared__ float R[kPosMaxOH];
  __shared__ float Q[kPosMaxOW];
  const int tid = threadIdx.x, lt = tid & 255, gq = tid >> 8, oc = blockIdx.x, OC = gridDim.x;
  const int cpg = (chunks + kPosFinGroups - 1) / kPosFinGroups, c0 = gq * cpg, c1 = min(chunks, c0 + cpg);
  for (int e = lt; e < OH + OW; e += 256) {
    const bool row = e < OH;
    const float* p = row ? partR + (long)oc * OH + e : partQ + (long)oc * OW + (e - OH);
    const long step = (long)OC * (row ? OH : OW);
    float acc = 0.f;
#pragma unroll 4
    for (int c = c0; c < c1; ++c) acc += p[c * step];
    red[gq][e] = acc;
  }
  __syncthreads();
  for (int e = tid; e < OH + OW; e += 256 * kPosFinGroups) {
    const float v = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    if (e < OH) R[e] = v;
    else Q[e - OH] = v;
  }
  __syncthreads();
  if (tid >= 2 * K) return;
  const int which = tid / K, k = tid - which * K;
  float* o = dw + (long)oc * dw_stride + (long)which * K * K;
  float acc = 0.f;
  if (which == 0) {
    for (int oy = 0; oy < OH; ++oy) acc = fmaf(pos_lin(S * oy + k, IH), R[oy], acc);
    for (int kx = 0; kx < K; ++kx) o[k * K + kx] = acc;
  } else {
    for (int ox = 0; ox < OW; ++ox) acc = fmaf(pos_lin(S * ox + k, IW), Q[ox], acc);
    for (int ky = 0; ky < K; ++ky) o[ky * K + k] = acc;
  }
}

bool pos_geo_ok(int OC, int K, int S, int IH, int IW, int* OH, int* OW) {
  if (OC <= 0 || K <= 0 || K > 16 || S <= 0 || IH < K || IW < K) return false;
  *OH = (IH - K) / S + 1;
  *OW = (IW - K) / S + 1;
  return *OH <= kPosMaxOH && *OW <= kPosMaxOW;
}

}  // namespace

int launch_pos_bias(int OC, int IC_total, int C, int K, int S, int IH, int IW, const float* W, float* rowb,
                    float* colb, hipStream_t s) {
  int OH, OW;
  if (!pos_geo_ok(OC, K, S, IH, IW, &OH, &OW) || C < 0 || IC_total < C + 2) return -1;
  hipLaunchKernelGGL(k_pos_bias, dim3((OC * (OH + OW) + 255) / 256), dim3(256), 0, s, W, OC, IC_total, C, K, S, IH, IW,
                     OH, OW, rowb, colb);
  return 0;
}

size_t pos_part_floats(int max_n, int OC, int OH, int OW) {
  return (size_t)((max_n + kPosSPC - 1) / kPosSPC) * OC * (OH + OW);
}

int launch_pos_wgrad(int n, int OC, int OH, int OW, int K, int S, int IH, int IW, const float* dz, long dz_stride,
                     float* dw, long dw_stride, float* part, size_t part_cap, hipStream_t s) {
  int oh, ow;
  if (n <= 0 || !pos_geo_ok(OC, K, S, IH, IW, &oh, &ow) || oh != OH || ow != OW) return -1;
  if (pos_part_floats(n, OC, OH, OW) > part_cap) return -1;
  const int chunks = (n + kPosSPC - 1) / kPosSPC;
  float* partR = part;
  float* partQ = part + (size_t)chunks * OC * OH;
  hipLaunchKernelGGL(k_pos_rq, dim3(chunks, OC), dim3(256), 0, s, dz, dz_stride, n, OH, OW, partR, partQ);
  hipLaunchKernelGGL(k_pos_wfin, dim3(OC), dim3(256 * kPosFinGroups), 0, s, partR, partQ, chunks, OH, OW, K, S, IH, IW, dw, dw_stride);
  return 0;
}

// ------------------------------------------------------------------------------------------
// test hooks (ppo_carla.h)
// ------------------------------------------------------------------------------------------
extern "C" int ppo_carla_debug_pos_grid(int n, float* host) {
  if (n <= 0 || !host) return ppo_fail("ppo_carla_debug_pos_grid: n must be positive, host not null", -1);
  for (int i = 0; i < n; ++i) host[i] = pos_lin(i, n);
  return 0;
}

extern "C" int ppo_carla_debug_pos_bias(int OC, int IC_total, int C, int K, int S, int IH, int IW, const float* W_dev,
                                        float* rowb_dev, float* colb_dev, void* stream) {
  if (!W_dev || !rowb_dev || !colb_dev) return ppo_fail("ppo_carla_debug_pos_bias: null argument", -1);
  int OH, OW;
  if (!pos_geo_ok(OC, K, S, IH, IW, &OH, &OW) || C < 0 || IC_total < C + 2)
    return ppo_fail("ppo_carla_debug_pos_bias: needs OC > 0, 0 < K <= 16, S > 0, IH, IW >= K, at most " +
                    std::to_string(kPosMaxOH) + " x " + std::to_string(kPosMaxOW) + " outputs, IC_total >= C + 2", -1);
  if (int rc = ppo_runtime_check()) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int fit = launch_pos_bias(OC, IC_total, C, K, S, IH, IW, W_dev, rowb_dev, colb_dev, s);
  if (fit != 0 || hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return ppo_fail("ppo_carla_debug_pos_bias: launch failed", -2);
  return 0;
}

extern "C" int ppo_carla_debug_pos_wgrad(int n, int max_n, int OC, int OH, int OW, int K, int S, int IH, int IW,
                                         const float* dz_dev, float* dw_pos_dev, void* stream) {
  if (!dz_dev || !dw_pos_dev) return ppo_fail("ppo_carla_debug_pos_wgrad: null argument", -1);
  int oh, ow;
  if (n <= 0 || max_n < n || !pos_geo_ok(OC, K, S, IH, IW, &oh, &ow) || oh != OH || ow != OW)
    return ppo_fail("ppo_carla_debug_pos_wgrad: needs 0 < n <= max_n, OC > 0, 0 < K <= 16, S > 0, OH x OW the "
                    "outputs of IH x IW (at most " + std::to_string(kPosMaxOH) + " x " + std::to_string(kPosMaxOW) + ")",
                    -1);
  if (int rc = ppo_runtime_check()) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* part = nullptr;
  const size_t part_cap = pos_part_floats(max_n, OC, OH, OW);
  if (hipMalloc((void**)&part, part_cap * sizeof(float)) != hipSuccess)
    return ppo_fail("ppo_carla_debug_pos_wgrad: device allocation failed", -2);
  const int fit = launch_pos_wgrad(n, OC, OH, OW, K, S, IH, IW, dz_dev, (long)OC * OH * OW, dw_pos_dev, 2L * K * K,
                                   part, part_cap, s);
  const bool ok = fit == 0 && hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  (void)hipFree(part);
  return ok ? 0 : ppo_fail("ppo_carla_debug_pos_wgrad: launch failed", -2);
}
