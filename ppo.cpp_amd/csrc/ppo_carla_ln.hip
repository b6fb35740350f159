// ppo_carla_ln.hip — the CaRL agent's LayerNorm + ReLU, forward and backward, and the test hooks that run
// them on caller arrays.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "ppo_carla_units.hpp"

namespace {

// ==========================================================================================
// LayerNorm + ReLU (carla_model.h:44-64 roach_ln, :113-175 use_layer_norm; nn::LayerNorm defaults:
// biased variance, eps 1e-5, per-element weight / bias shared over rows). A normalised layer's
// convolution / Linear runs with relu = 0 into a pre-activation buffer z and k_carla_ln writes
// relu(x^ * gamma + beta) where the layer's output goes today, so the next layer and every gradient
// kernel see what they see without LayerNorm. All kernels are memory-bound row or column sweeps;
// every sum is a per-thread strided loop and an LDS tree: a fixed order, no atomics.
// ==========================================================================================
constexpr float kLnEps = 1e-5f;

template <int T = 256>
PPO_DEV float ln_block_sum(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = T / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// One row per workgroup: mean, then the variance about that mean (second sweep), then y (third).
// VEC: 16-byte loads / stores of z and y (F and both strides multiples of 4, both bases 16-byte
// aligned); gamma / beta sit at arbitrary float offsets of the parameter vector.
template <bool VEC>
__global__ __launch_bounds__(256) void k_carla_ln(const float* __restrict__ in, long in_stride, float* __restrict__ out,
                                                  long out_stride, int F, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, float* __restrict__ stat) {
  __shared__ float red[256];
  const long r = blockIdx.x;
  const float* z = in + r * in_stride;
  float* y = out + r * out_stride;
  float s = 0.f;
  if (VEC) {
    const float4* z4 = reinterpret_cast<const float4*>(z);
    for (int i = threadIdx.x; i < F / 4; i += 256) {
      const float4 v = z4[i];
      s += (v.x + v.y) + (v.z + v.w);
    }
  } else {
    for (int i = threadIdx.x; i < F; i += 256) s += z[i];
  }
  const float mean0 = ln_block_sum(s, red) / (float)F;
  // corrected two-pass (Chan, Golub, LeVeque): the second sweep also sums the residuals z - mean0,
  // which carry the rounding error of the first sum; mean = mean0 + e, var = sum (z - mean0)^2 / F - e^2
  float q = 0.f, e1 = 0.f;
  if (VEC) {
    const float4* z4 = reinterpret_cast<const float4*>(z);
    for (int i = threadIdx.x; i < F / 4; i += 256) {
      const float4 v = z4[i];
      const float a = v.x - mean0, b = v.y - mean0, c = v.z - mean0, d = v.w - mean0;
      q += (a * a + b * b) + (c * c + d * d);
      e1 += (a + b) + (c + d);
    }
  } else {
    for (int i = threadIdx.x; i < F; i += 256) {
      const float a = z[i] - mean0;
      q += a * a;
      e1 += a;
    }
  }
  const float e = ln_block_sum(e1, red) / (float)F;
  const float mean = mean0 + e;
  const float rstd = 1.0f / sqrtf(fmaxf(ln_block_sum(q, red) / (float)F - e * e, 0.f) + kLnEps);
  if (threadIdx.x == 0) {
    stat[2 * r] = mean;
    stat[2 * r + 1] = rstd;
  }
  if (VEC) {
    const float4* z4 = reinterpret_cast<const float4*>(z);
    float4* y4 = reinterpret_cast<float4*>(y);
    for (int i = threadIdx.x; i < F / 4; i += 256) {
      const float4 v = z4[i];
      const float* g = gamma + 4 * i;
      const float* b = beta + 4 * i;
      float4 o;
      o.x = fmaxf((v.x - mean) * rstd * g[0] + b[0], 0.f);
      o.y = fmaxf((v.y - mean) * rstd * g[1] + b[1], 0.f);
      o.z = fmaxf((v.z - mean) * rstd * g[2] + b[2], 0.f);
      o.w = fmaxf((v.w - mean) * rstd * g[3] + b[3], 0.f);
      y4[i] = o;
    }
  } else {
    for (int i = threadIdx.x; i < F; i += 256) y[i] = fmaxf((z[i] - mean) * rstd * gamma[i] + beta[i], 0.f);
  }
}

// The same for long rows (F >= kLnBigMin, vector-aligned): at training batch sizes every row is in flight
// at once (2 048 x 283 KB against 32 MB of L2), so k_carla_ln's second and third sweeps would come from
// HBM again. Here a workgroup of 1 024 threads keeps its row in registers (NV float4 per thread, F <=
// 4 096 NV): one read, one write. Same arithmetic per element; the sums take another (fixed) order.
constexpr int kLnBigThreads = 1024, kLnBigMin = 4096, kLnBigMaxVec = 18;

template <int NV>
__global__ __launch_bounds__(kLnBigThreads) void k_carla_ln_big(const float* __restrict__ in, long in_stride,
                                                                float* __restrict__ out, long out_stride, int F,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta,
                                                                float* __restrict__ stat) {
  __shared__ float red[kLnBigThreads];
  const long r = blockIdx.x;
  const float4* z4 = reinterpret_cast<const float4*>(in + r * in_stride);
  float4* y4 = reinterpret_cast<float4*>(out + r * out_stride);
  const int F4 = F / 4;
  float4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = k * kLnBigThreads + threadIdx.x;
    v[k] = i < F4 ? z4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
  }
  const float mean0 = ln_block_sum<kLnBigThreads>(s, red) / (float)F;
  float q = 0.f, e1 = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    if (k * kLnBigThreads + (int)threadIdx.x < F4) {
      const float a = v[k].x - mean0, b = v[k].y - mean0, c = v[k].z - mean0, d = v[k].w - mean0;
      q += (a * a + b * b) + (c * c + d * d);
      e1 += (a + b) + (c + d);
    }
  }
  const float e = ln_block_sum<kLnBigThreads>(e1, red) / (float)F;
  const float mean = mean0 + e;
  const float rstd = 1.0f / sqrtf(fmaxf(ln_block_sum<kLnBigThreads>(q, red) / (float)F - e * e, 0.f) + kLnEps);
  if (threadIdx.x == 0) {
    stat[2 * r] = mean;
    stat[2 * r + 1] = rstd;
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int i = k * kLnBigThreads + threadIdx.x;
    if (i < F4) {
      const float* g = gamma + 4 * i;
      const float* b = beta + 4 * i;
      float4 o;
      o.x = fmaxf((v[k].x - mean) * rstd * g[0] + b[0], 0.f);
      o.y = fmaxf((v[k].y - mean) * rstd * g[1] + b[1], 0.f);
      o.z = fmaxf((v[k].z - mean) * rstd * g[2] + b[2], 0.f);
      o.w = fmaxf((v[k].w - mean) * rstd * g[3] + b[3], 0.f);
      y4[i] = o;
    }
  }
}

// Row pass of the backward, in place: d holds dy * [y > 0] on entry (the consuming layer's
// input-gradient kernel applied the mask) and dz = rstd * (g - a - x^ * b) on exit, with g = d * gamma,
// a = sum g / F, b = sum g x^ / F. Each thread rewrites only the elements it read in the second sweep.
template <bool VEC>
__global__ __launch_bounds__(256) void k_carla_ln_bwd(float* __restrict__ d, long d_stride,
                                                      const float* __restrict__ zin, long z_stride, int F,
                                                      const float* __restrict__ gamma,
                                                      const float* __restrict__ stat) {
  __shared__ float red[256];
  const long r = blockIdx.x;
  float* dr = d + r * d_stride;
  const float* z = zin + r * z_stride;
  const float mean = stat[2 * r], rstd = stat[2 * r + 1];
  float sa = 0.f, sb = 0.f;
  if (VEC) {
    const float4* z4 = reinterpret_cast<const float4*>(z);
    const float4* d4 = reinterpret_cast<const float4*>(dr);
    for (int i = threadIdx.x; i < F / 4; i += 256) {
      const float4 v = z4[i], dv = d4[i];
      const float* g = gamma + 4 * i;
      const float g0 = dv.x * g[0], g1 = dv.y * g[1], g2 = dv.z * g[2], g3 = dv.w * g[3];
      sa += (g0 + g1) + (g2 + g3);
      sb += (g0 * ((v.x - mean) * rstd) + g1 * ((v.y - mean) * rstd)) +
            (g2 * ((v.z - mean) * rstd) + g3 * ((v.w - mean) * rstd));
    }
  } else {
    for (int i = threadIdx.x; i < F; i += 256) {
      const float g = dr[i] * gamma[i];
      sa += g;
      sb += g * ((z[i] - mean) * rstd);
    }
  }
  const float a = ln_block_sum(sa, red) / (float)F;
  const float b = ln_block_sum(sb, red) / (float)F;
  if (VEC) {
    const float4* z4 = reinterpret_cast<const float4*>(z);
    float4* d4 = reinterpret_cast<float4*>(dr);
    for (int i = threadIdx.x; i < F / 4; i += 256) {
      const float4 v = z4[i], dv = d4[i];
      const float* g = gamma + 4 * i;
      float4 o;
      o.x = rstd * (dv.x * g[0] - a - (v.x - mean) * rstd * b);
      o.y = rstd * (dv.y * g[1] - a - (v.y - mean) * rstd * b);
      o.z = rstd * (dv.z * g[2] - a - (v.z - mean) * rstd * b);
      o.w = rstd * (dv.w * g[3] - a - (v.w - mean) * rstd * b);
      d4[i] = o;
    }
  } else {
    for (int i = threadIdx.x; i < F; i += 256) dr[i] = rstd * (dr[i] * gamma[i] - a - (z[i] - mean) * rstd * b);
  }
}

// Column pass: dgamma[e] = sum over rows d * x^, dbeta[e] = sum over rows d (d = dy * [y > 0], so this
// runs before the in-place row pass). blockIdx.y = a chunk of rpc consecutive rows, a thread = one
// element (coalesced over e); part [chunks][2][F]. k_carla_ln_dgb_sum adds the chunks in order, as
// k_wsum does for the weight gradients.
__global__ __launch_bounds__(256) void k_carla_ln_dgb(const float* __restrict__ d, long d_stride,
                                                      const float* __restrict__ z, long z_stride, int n, int F,
                                                      int rpc, const float* __restrict__ stat,
                                                      float* __restrict__ part) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= F) return;
  const int r0 = blockIdx.y * rpc, r1 = r0 + rpc < n ? r0 + rpc : n;
  float dg = 0.f, db = 0.f;
  for (int r = r0; r < r1; ++r) {
    const float dv = d[(long)r * d_stride + e];
    dg += dv * ((z[(long)r * z_stride + e] - stat[2 * r]) * stat[2 * r + 1]);
    db += dv;
  }
  part[((long)blockIdx.y * 2) * F + e] = dg;
  part[((long)blockIdx.y * 2 + 1) * F + e] = db;
}

__global__ __launch_bounds__(256) void k_carla_ln_dgb_sum(const float* __restrict__ part, int chunks, int F,
                                                          float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= F) return;
  float dg = 0.f, db = 0.f;
  for (int c = 0; c < chunks; ++c) {
    dg += part[((long)c * 2) * F + e];
    db += part[((long)c * 2 + 1) * F + e];
  }
  dgamma[e] = dg;
  dbeta[e] = db;
}

// (hook only) what the consuming layer's input-gradient kernel does in the agent: d = dy * [y > 0]
__global__ void k_carla_ln_mask(const float* __restrict__ dy, const float* __restrict__ y, long y_stride, int n, int F,
                                float* __restrict__ d) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)n * F) return;
  const long r = i / F;
  d[i] = y[r * y_stride + (i - r * F)] > 0.0f ? dy[i] : 0.0f;
}

}  // namespace

// column-pass chunks aimed at for n rows: about 1024 workgroups over (column blocks x chunks), at most
// 64 and at most n. Non-decreasing in n.
static int ln_max_chunks(int n, int F) {
  const int cb = (F + 255) / 256;
  return std::max(1, std::min((1024 + cb - 1) / cb, std::min(n, 64)));
}
static int ln_rows_per_chunk(int n, int F) {
  const int chunks = ln_max_chunks(n, F);
  return (n + chunks - 1) / chunks;
}
// Partial-sum floats that serve every batch of up to max_n rows. The chunks a batch of n rows really
// uses, ceil(n / rows per chunk), are at most ln_max_chunks(n) <= ln_max_chunks(max_n), but not
// monotone in n, so the buffer is sized by that bound and not by max_n's own chunk count.
size_t ln_part_floats(int max_n, int F) { return (size_t)ln_max_chunks(max_n, F) * 2 * F; }

static bool ln_vec_ok(const void* a, long as, const void* b, long bs, int F) {
  return F % 4 == 0 && as % 4 == 0 && bs % 4 == 0 && (reinterpret_cast<uintptr_t>(a) & 15) == 0 &&
         (reinterpret_cast<uintptr_t>(b) & 15) == 0;
}

void launch_ln_fwd(int n, int F, const float* z, long zs, const float* gamma, const float* beta, float* y, long ys,
                   float* stat, hipStream_t s) {
  const bool vec = ln_vec_ok(z, zs, y, ys, F);
  const int nv = (F / 4 + kLnBigThreads - 1) / kLnBigThreads;
#define PPO_LN_BIG(NV_) \
  hipLaunchKernelGGL((k_carla_ln_big<NV_>), dim3(n), dim3(kLnBigThreads), 0, s, z, zs, y, ys, F, gamma, beta, stat)
  if (vec && F >= kLnBigMin && nv <= kLnBigMaxVec) {
    if (nv <= 2) PPO_LN_BIG(2);
    else if (nv <= 4) PPO_LN_BIG(4);
    else if (nv <= 8) PPO_LN_BIG(8);
    else PPO_LN_BIG(kLnBigMaxVec);
  } else if (vec) {
    hipLaunchKernelGGL((k_carla_ln<true>), dim3(n), dim3(256), 0, s, z, zs, y, ys, F, gamma, beta, stat);
  } else {
    hipLaunchKernelGGL((k_carla_ln<false>), dim3(n), dim3(256), 0, s, z, zs, y, ys, F, gamma, beta, stat);
  }
#undef PPO_LN_BIG
}

// d [n][F] (stride ds): dy * [y > 0] in, dz out; part holds part_cap floats (ln_part_floats of the largest
// batch). Returns -1, launching nothing, if this batch's chunks would not fit.
int launch_ln_bwd(int n, int F, float* d, long ds, const float* z, long zs, const float* gamma, const float* stat,
                  float* dgamma, float* dbeta, float* part, size_t part_cap, hipStream_t s) {
  const int rpc = ln_rows_per_chunk(n, F), chunks = (n + rpc - 1) / rpc, cb = (F + 255) / 256;
  if ((size_t)chunks * 2 * F > part_cap) return -1;
  hipLaunchKernelGGL(k_carla_ln_dgb, dim3(cb, chunks), dim3(256), 0, s, d, ds, z, zs, n, F, rpc, stat, part);
  hipLaunchKernelGGL(k_carla_ln_dgb_sum, dim3(cb), dim3(256), 0, s, part, chunks, F, dgamma, dbeta);
  if (ln_vec_ok(d, ds, z, zs, F))
    hipLaunchKernelGGL((k_carla_ln_bwd<true>), dim3(n), dim3(256), 0, s, d, ds, z, zs, F, gamma, stat);
  else
    hipLaunchKernelGGL((k_carla_ln_bwd<false>), dim3(n), dim3(256), 0, s, d, ds, z, zs, F, gamma, stat);
  return 0;
}

// ------------------------------------------------------------------------------------------
// test hooks: the agent's LayerNorm launches on caller arrays (ppo_carla.h)
// ------------------------------------------------------------------------------------------
extern "C" int ppo_carla_debug_ln_forward(int n, int F, const float* z, long in_stride, const float* gamma,
                                          const float* beta, float* y, long out_stride, float* stat, void* stream) {
  if (!z || !gamma || !beta || !y || !stat) return ppo_fail("ppo_carla_debug_ln_forward: null argument", -1);
  if (n <= 0 || F <= 0 || in_stride < F || out_stride < F)
    return ppo_fail("ppo_carla_debug_ln_forward: n and F must be positive, strides at least F", -1);
  if (int rc = ppo_runtime_check()) return rc;
  launch_ln_fwd(n, F, z, in_stride, gamma, beta, y, out_stride, stat, (hipStream_t)stream);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return ppo_fail("ppo_carla_debug_ln_forward: launch failed", -2);
  return 0;
}

extern "C" int ppo_carla_debug_ln_backward(int n, int F, const float* z, long in_stride, const float* gamma,
                                           const float* stat, const float* y, long out_stride, const float* dy,
                                           float* dz, float* dgamma, float* dbeta, void* stream) {
  if (!z || !gamma || !stat || !y || !dy || !dz || !dgamma || !dbeta)
    return ppo_fail("ppo_carla_debug_ln_backward: null argument", -1);
  if (n <= 0 || F <= 0 || in_stride < F || out_stride < F)
    return ppo_fail("ppo_carla_debug_ln_backward: n and F must be positive, strides at least F", -1);
  if (int rc = ppo_runtime_check()) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* part = nullptr;
  const size_t part_cap = ln_part_floats(n, F);
  if (hipMalloc((void**)&part, part_cap * sizeof(float)) != hipSuccess)
    return ppo_fail("ppo_carla_debug_ln_backward: device allocation failed", -2);
  const long tot = (long)n * F;
  hipLaunchKernelGGL(k_carla_ln_mask, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, dy, y, out_stride, n, F,
                     dz);
  const int fit = launch_ln_bwd(n, F, dz, F, z, in_stride, gamma, stat, dgamma, dbeta, part, part_cap, s);
  const bool ok = fit == 0 && hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  (void)hipFree(part);
  return ok ? 0 : ppo_fail("ppo_carla_debug_ln_backward: launch failed", -2);
}
