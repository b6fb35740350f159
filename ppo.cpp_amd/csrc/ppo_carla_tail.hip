// ppo_carla_tail.hip — what follows the CNN in the CaRL agent's forward (carla_model.h:238-284):
// k_carla_pack, k_carla_head and, at rollout batch sizes, the whole MLP part as k_carla_tail.
//
//  * k_carla_head: dist_mu / dist_sigma dot products, softplus + beta_min, the Beta sample (the
//    Philox / Marsaglia-Tsang contract of the MLP agents), mean, roach_deterministic or the given
//    action, log_prob and entropy (rl_utils.h:87-132), one thread per row.
#include <hip/hip_runtime.h>

#include "ppo_carla_units.hpp"
#include "ppo_dist.hpp"

namespace {

// value_measurements -> columns [256, 256 + NV) of the value-head input (carla_model.h:276)
__global__ void k_carla_pack(const float* __restrict__ vmeas, float* __restrict__ feat, int n, int NV) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * NV) return;
  const int r = i / NV, c = i - r * NV;
  feat[(long)r * (256 + NV) + 256 + c] = vmeas[i];
}

// A value the compiler may not look through: the per-concentration results (gamma draw, lgamma,
// digamma) are computed by other threads in the fused tail's head (tail_head_rows) and reach the
// combining expressions through LDS; the same barrier here keeps the two paths' fp contraction (a
// producer's final multiply fused into its consumer's add) identical, so they agree bit for bit.
// beta_unit (ppo_dist.hpp) switches on PPO_GIVEN / PPO_MEAN / PPO_ROACH; this file passes it PPO_CARLA_* modes
static_assert((int)PPO_CARLA_SAMPLE == (int)PPO_SAMPLE && (int)PPO_CARLA_MEAN == (int)PPO_MEAN &&
                  (int)PPO_CARLA_GIVEN == (int)PPO_GIVEN && (int)PPO_CARLA_ROACH == (int)PPO_ROACH,
              "the CaRL sample types must be the MLP agents' values");

PPO_DEV float opaque_(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

// The Beta head's arithmetic in two pieces shared by k_carla_head (one thread per row) and the fused
// tail (tail_head_rows: the pieces on different threads, exchanged through LDS). Every value that
// crosses from one piece to the other, and every transcendental result, passes opaque_, so both
// paths compile the same expression trees over the same leaves (no contraction into a consumer
// in one path only) and agree bit for bit.
struct BetaConc {
  float conc, draw, lg, dg;  // softplus(pre) + beta_min, its gamma draw (sampling), lgamma, digamma
};
PPO_DEV BetaConc beta_conc(const HeadArgs& h, float pre, SampleKey key, long env, int ai, int side) {
  BetaConc c;
  c.conc = opaque_(opaque_(softplusf_(pre)) + h.beta_min);
  c.draw = h.mode == PPO_CARLA_SAMPLE
               ? opaque_(gamma_mt(c.conc, key, env, h.step_id, 0x10000u + (uint32_t)(ai * 2 + side) * 64u))
               : 0.0f;
  c.lg = opaque_(lgammaf(c.conc));
  c.dg = opaque_(digammaf_(c.conc));
  return c;
}
// action ai of row r: the sample / mean / roach / given value and the action's log-prob and
// entropy terms (carla_head_row adds them over actions in action order); writes action / alpha / beta
PPO_DEV void carla_beta_terms(const HeadArgs& h, int r, int ai, const BetaConc& ca, const BetaConc& cb, float& lpt,
                         float& entt) {
  const float* P = h.P;
  const float hi = P[h.hi], lo = P[h.lo];
  const float al = ca.conc, be = cb.conc;
  float given = 0.f;
  if (h.mode == PPO_CARLA_GIVEN) given = beta_unit_from_action(h.action_in[(long)r * h.A + ai], lo, hi);
  const float sv = opaque_(beta_unit(h.mode, al, be, ca.draw, cb.draw, given));
  const float ab = al + be;
  const float lgab = opaque_(lgammaf(ab)), dgab = opaque_(digammaf_(ab));
  // the two terms keep their own text: the opaque_ barriers sit inside the expressions
  const float xa = opaque_(xlogyf_(al - 1.0f, sv)), xb = opaque_(xlogyf_(be - 1.0f, 1.0f - sv));
  lpt = opaque_(xa + xb + (lgab - (ca.lg + cb.lg)));
  entt = opaque_((ca.lg + cb.lg) - lgab - (2.0f - ab) * dgab - ((al - 1.0f) * ca.dg + (be - 1.0f) * cb.dg));
  if (h.action) h.action[(long)r * h.A + ai] = beta_action(sv, lo, hi);
  if (h.alpha) h.alpha[(long)r * h.A + ai] = al;
  if (h.beta) h.beta[(long)r * h.A + ai] = be;
}

// one row of k_carla_head: the dist_mu / dist_sigma dot products (or, with pre != nullptr, their
// values computed by the same loop elsewhere: pre[ai] = mu, pre[A + ai] = sigma pre-activations),
// softplus + beta_min, the sample / mean / roach / given value, log_prob, entropy
PPO_DEV void carla_head_row(const HeadArgs& h, int r, const float* pre, bool copy_value) {
  const float* P = h.P;
  const float* x = h.latent + (long)r * 256;
  const SampleKey key = sample_key(h.seed, h.rank);
  const long env = h.env_base + r;
  float lp = 0.f, ent = 0.f;
  for (int ai = 0; ai < h.A; ++ai) {
    float pm, ps;
    if (pre) {
      pm = pre[ai];
      ps = pre[h.A + ai];
    } else {
      const float* wm = P + h.mu_w + (long)ai * 256;
      const float* ws = P + h.sg_w + (long)ai * 256;
      pm = 0.f;
      ps = 0.f;
      for (int k = 0; k < 256; ++k) {
        pm = fmaf(wm[k], x[k], pm);
        ps = fmaf(ws[k], x[k], ps);
      }
      pm += P[h.mu_b + ai];
      ps += P[h.sg_b + ai];
    }
    if (h.hpre) {
      h.hpre[(long)r * 2 * h.A + ai] = pm;
      h.hpre[(long)r * 2 * h.A + h.A + ai] = ps;
    }
    const BetaConc ca = beta_conc(h, pm, key, env, ai, 0), cb = beta_conc(h, ps, key, env, ai, 1);
    float lpt, entt;
    carla_beta_terms(h, r, ai, ca, cb, lpt, entt);
    lp += lpt;
    ent += entt;
  }
  if (h.logprob) h.logprob[r] = lp;
  if (h.entropy) h.entropy[r] = ent;
  if (copy_value && h.value) h.value[r] = h.val[r];
}

__global__ __launch_bounds__(64) void k_carla_head(HeadArgs h) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= h.n) return;
  carla_head_row(h, r, nullptr, true);
}

// ==========================================================================================
// The MLP tail at rollout batch sizes (n <= kTailMaxN): state MLP, linear, value and policy heads
// and the distribution head after the CNN, as stages of ONE kernel (cooperative launch, a grid
// barrier between stages) instead of ~20 launches of k_conv / k_conv_fin / k_carla_pack /
// k_carla_head, whose fixed cost per launch dominated the 32-row forward. Every Linear output is
// bitwise k_conv's: a work item (16 rows x 16 output channels of one layer) is one workgroup, its
// waves run the same MFMA chains over the same 128-wide k chunks (same operands, same step order,
// same masked operands), and the chunk partials are added in z order from 0 as k_conv_fin does
// (one chunk: acc + bias, as k_conv). The head's dot products run one (row, action) per thread with
// k_carla_head's loop; the per-row Beta arithmetic is k_carla_head's.
// ==========================================================================================
constexpr int kTailThreads = 512, kTailMaxZ = 10, kTailMaxLin = 9, kTailMaxStage = 8;
constexpr int kTailLdx = 256 + 4;  // LDS row stride of a recomputed layer's output (OC <= 256)
constexpr int kTailPreMaxK = 32;   // widest input of a layer computed inside its consumer's items

struct TailLin {
  const float* in;
  long in_stride;
  int K;
  long w, b;  // parameter offsets: W [OC][K], b [OC]
  float* out;
  long out_stride;
  int OC, relu;
  float* out2;  // optional copy of output column 0 (the value head's last layer -> value), stride 1
};
struct TailArgs {
  const float* P;
  int n;
  ConvArgs c6;  // conv6's split-K partials, finished in stage 0 as k_conv_fin (c6_Z > 1)
  int c6_Z;
  const float* vmeas;  // value measurements -> feat columns [256, 256 + NV) (stage 0)
  float* feat;
  int NV;
  TailLin lin[kTailMaxLin];
  int lin_stage[kTailMaxLin];  // stage of each layer (non-decreasing)
  int nlin, nstage, head_stage;
  HeadArgs h;
  unsigned* bar;       // grid barrier counter (monotonic across launches)
  unsigned bar_base;   // its value when this launch started
  int stage_lo, stage_hi;  // the stages this launch runs (a barrier between consecutive ones)
  int pre_lin, pre_for;    // layer pre_lin (K < 256, stage -1) is computed inside layer pre_for's items
                           // for their rows (LDS), instead of as a stage of its own; -1: none
};

PPO_DEV int tail_z(int K) { return K >= 256 ? (K + kSplitKC - 1) / kSplitKC : 1; }

// one Linear work item: rows s0 .. s0 + 15, output channels oc0 .. oc0 + 15 of layer L
// (in_row0: the row of the batch that L.in's row 0 holds — 0 for a global input, s0 for rows staged in LDS)
PPO_DEV void tail_lin_item(const float* __restrict__ P, const TailLin& L, int n, int s0, int oc0, float* part,
                           int in_row0 = 0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const int K = L.K, Z = tail_z(K), kc = Z > 1 ? kSplitKC : K;
  const int oc = oc0 + j, s = s0 + j;
  const float* wrow = P + L.w + (long)(oc < L.OC ? oc : 0) * K;
  const bool sv = s < n;
  const float* xrow = L.in + (long)(sv ? s - in_row0 : 0) * L.in_stride;
  // a chunk is at most 32 k-steps (128 / 4): all 64 operand loads of a lane go out together (one
  // memory latency per chunk), from clamped addresses, masked afterwards (issuing a second chunk's
  // loads before the first chunk's chain, for linear.0's ten chunks on eight waves, measured slower:
  // 236 VGPRs)
  constexpr int NW = kTailThreads / 64, NU = kSplitKC / 4;
  auto load = [&](int z, float (&av)[NU], float (&bv)[NU]) {
    const int kbeg = z * kc, kend = min(K, kbeg + kc);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int k = kbeg + 4 * u + g;
      // k_conv's staged weight: rows of K % 4 == 0 are read as float4s from min(k, K - 4), so a
      // masked tap past the end holds W[K - 4 + (k & 3)]; other rows clamp to K - 1
      const int kw = (K & 3) == 0 ? (k < K ? k : K - 4 + (k & 3)) : min(k, K - 1);
      av[u] = wrow[kw] * ((oc < L.OC && k < kend) ? 1.0f : 0.0f);
      const bool ok = sv && k < kend;
      bv[u] = (ok ? xrow[min(k, K - 1)] : L.in[0]) * (ok ? 1.0f : 0.0f);
    }
  };
  auto chain = [&](int z, const float (&av)[NU], const float (&bv)[NU]) {
    const int kbeg = z * kc, kend = min(K, kbeg + kc);
    const int nsteps = 4 * ((kend - kbeg + 15) / 16);
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (u < nsteps) acc = mfma16(av[u], bv[u], acc);
    // lane (j, g) holds output channel oc0 + 4 g + r of row s0 + j
#pragma unroll
    for (int r = 0; r < 4; ++r) part[(z * 16 + 4 * g + r) * 17 + j] = acc[r];
  };
  for (int z = wave; z < Z; z += NW) {
    float av[NU], bv[NU];
    load(z, av, bv);
    chain(z, av, bv);
  }
  __syncthreads();
  if (tid < 256) {
    const int ocl = tid >> 4, sl = tid & 15, o = oc0 + ocl, r = s0 + sl;
    if (o < L.OC && r < n) {
      float y;
      if (Z == 1) {
        y = part[ocl * 17 + sl] + P[L.b + o];
      } else {
        float v = 0.f;
        for (int z = 0; z < Z; ++z) v += part[(z * 16 + ocl) * 17 + sl];
        y = v + P[L.b + o];
      }
      if (L.relu) y = y > 0.0f ? y : 0.0f;
      L.out[(long)r * L.out_stride + o] = y;
      if (L.out2 && o == 0) L.out2[r] = y;
    }
  }
  __syncthreads();  // part is reused by the next item
}

// All OC outputs of a one-chunk layer L (K < 256) for rows s0 .. s0 + 15 into LDS xs[16][ldx], with
// tail_lin_item's arithmetic (per 16x16 tile the same MFMA chain over the same masked operands, then
// + bias, relu), so a dependent layer's items can take them as their input without a stage of their
// own (the state MLP's first layer under its second). Optionally also stored to L.out (rows < n).
PPO_DEV void tail_lin_rows_lds(const float* __restrict__ P, const TailLin& L, int n, int s0, float* xs, int ldx,
                               bool store) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  constexpr int NU = kTailPreMaxK / 4;  // u-steps a K <= kTailPreMaxK layer can use (tail_lin_item loads
                                        // kSplitKC / 4 and issues the first nsteps: the same operands)
  const int K = L.K, kend = K;
  const int nsteps = 4 * ((K + 15) / 16);
  const int s = s0 + j;
  const bool sv = s < n;
  const float* xrow = L.in + (long)(sv ? s : 0) * L.in_stride;
#pragma unroll 1
  for (int ot = wave; ot < (L.OC + 15) / 16; ot += kTailThreads / 64) {
    const int oc0 = 16 * ot, oc = oc0 + j;
    const float* wrow = P + L.w + (long)(oc < L.OC ? oc : 0) * K;
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
    float av[NU], bv[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int k = 4 * u + g;
      const int kw = (K & 3) == 0 ? (k < K ? k : K - 4 + (k & 3)) : min(k, K - 1);
      av[u] = wrow[kw] * ((oc < L.OC && k < kend) ? 1.0f : 0.0f);
      const bool ok = sv && k < kend;
      bv[u] = (ok ? xrow[min(k, K - 1)] : L.in[0]) * (ok ? 1.0f : 0.0f);
    }
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (u < nsteps) acc = mfma16(av[u], bv[u], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = oc0 + 4 * g + r;
      if (o < L.OC) {
        float y = acc[r] + P[L.b + o];
        if (L.relu) y = y > 0.0f ? y : 0.0f;
        xs[j * ldx + o] = y;
        if (store && sv) L.out[(long)s * L.out_stride + o] = y;
      }
    }
  }
  __syncthreads();
}

// The tail's Beta head for rows r0 .. r0 + rows - 1 (rows * 2A <= kTailThreads), given the dist_mu /
// dist_sigma pre-activations pre[row][2A]: carla_head_row's arithmetic spread over threads — one per
// (row, concentration) for softplus, the gamma draw, lgamma and digamma of that concentration, one
// per (row, action) for the sample value and the action's log-prob / entropy terms, one per row for
// the sums over actions in action order (lp = (0 + t_0) + t_1 ..., as carla_head_row's loop adds
// them) — so the row's serial chain is one concentration plus one action instead of 2A of each.
PPO_DEV void tail_head_rows(const HeadArgs& h, int r0, int rows, const float* pre, float* hsc) {
  const int tid = threadIdx.x, A = h.A, n = h.n;
  const SampleKey key = sample_key(h.seed, h.rank);
  BetaConc* cs = reinterpret_cast<BetaConc*>(hsc);  // [rows][2A]
  {  // (row, q): q < A the alpha side of action q, q >= A the beta side of action q - A
    const int rl = tid / (2 * A), q = tid - rl * 2 * A, r = r0 + rl;
    if (rl < rows && r < n) {
      const int side = q < A ? 0 : 1, ai = q - side * A;
      const float x = pre[rl * 2 * A + q];
      if (h.hpre) h.hpre[(long)r * 2 * A + q] = x;
      cs[rl * 2 * A + q] = beta_conc(h, x, key, h.env_base + r, ai, side);
    }
  }
  __syncthreads();
  float* terms = hsc + kTailThreads * 4;  // [rows][A][2]: log-prob term, entropy term
  {
    const int rl = tid / A, ai = tid - rl * A, r = r0 + rl;
    if (rl < rows && r < n)
      carla_beta_terms(h, r, ai, cs[rl * 2 * A + ai], cs[rl * 2 * A + A + ai], terms[tid * 2], terms[tid * 2 + 1]);
  }
  __syncthreads();
  if (tid < rows && r0 + tid < n) {
    float lp = 0.f, ent = 0.f;
    for (int ai = 0; ai < A; ++ai) {
      lp += terms[(tid * A + ai) * 2 + 0];
      ent += terms[(tid * A + ai) * 2 + 1];
    }
    if (h.logprob) h.logprob[r0 + tid] = lp;
    if (h.entropy) h.entropy[r0 + tid] = ent;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kTailThreads) void k_carla_tail(TailArgs a) {
  __shared__ float part[kTailMaxZ * 16 * 17];
  __shared__ float pre[kTailThreads * 2];
  __shared__ float xs[16 * kTailLdx];            // rows of layer pre_lin, computed inside pre_for's items
  __shared__ float hsc[kTailThreads * 4 + kTailThreads * 2];  // head scratch (tail_head_rows)
  const int tid = threadIdx.x;
  const int rt_n = (a.n + 15) / 16;
  for (int stage = a.stage_lo; stage <= a.stage_hi; ++stage) {
    if (stage > a.stage_lo) grid_barrier(a.bar, a.bar_base + (unsigned)(stage - a.stage_lo) * gridDim.x);
    if (stage == 0) {  // conv6's split-K finish (k_conv_fin) and the value measurements
      const long gt = (long)blockIdx.x * kTailThreads + tid, gs = (long)gridDim.x * kTailThreads;
      if (a.c6_Z > 1) {
        const ConvArgs& c = a.c6;
        const int P6 = c.OH * c.OW;
        const long Q = (long)c.n * P6;
        for (long i = gt; i < Q * c.OC; i += gs) {
          const long q = i / c.OC;
          const int oc = (int)(i - q * c.OC);
          float v = 0.f;
          for (int z = 0; z < a.c6_Z; ++z) v += c.part[(size_t)z * Q * c.OC + i];
          float y = v + c.b[oc];
          if (c.relu) y = y > 0.0f ? y : 0.0f;
          const long smp = q / P6;
          c.out[smp * c.out_stride + (long)oc * P6 + (q - smp * P6)] = y;
        }
      }
      for (long i = gt; i < (long)a.n * a.NV; i += gs) {
        const long r = i / a.NV, cc = i - r * a.NV;
        a.feat[r * (256 + a.NV) + 256 + cc] = a.vmeas[i];
      }
    }
    // Linear work items of this stage, then (head stage) the distribution head
    int nitems = 0;
    for (int l = 0; l < a.nlin; ++l)
      if (a.lin_stage[l] == stage) nitems += rt_n * ((a.lin[l].OC + 15) / 16);
    const int head_wgs = stage == a.head_stage ? (a.n * a.h.A * 2 + kTailThreads - 1) / kTailThreads : 0;
    for (int it = blockIdx.x; it < nitems + head_wgs; it += gridDim.x) {
      if (it < nitems) {
        int rem = it, l = 0;
        for (; l < a.nlin; ++l) {
          if (a.lin_stage[l] != stage) continue;
          const int cnt = rt_n * ((a.lin[l].OC + 15) / 16);
          if (rem < cnt) break;
          rem -= cnt;
        }
        const int rt = rem % rt_n, ot = rem / rt_n;
        TailLin lx = a.lin[l];
        int row0 = 0;
        if (l == a.pre_for) {  // its input rows first, from the one-chunk layer pre_lin (ot 0 also stores them)
          tail_lin_rows_lds(a.P, a.lin[a.pre_lin], a.n, 16 * rt, xs, kTailLdx, ot == 0);
          lx.in = xs;
          lx.in_stride = kTailLdx;
          row0 = 16 * rt;
        }
        tail_lin_item(a.P, lx, a.n, 16 * rt, 16 * ot, part, row0);
      } else {
        // head: thread (row, ai, mu | sigma) runs k_carla_head's dot product loop for its
        // pre-activation; then one thread per row the rest of k_carla_head
        const HeadArgs& h = a.h;
        const int A = h.A, rows = kTailThreads / (2 * A), r0 = (it - nitems) * rows;
        const int rl = tid / (2 * A), q = tid - rl * 2 * A, r = r0 + rl;
        if (rl < rows && r < a.n) {
          const int ai = q < A ? q : q - A;
          const float* wv = a.P + (q < A ? h.mu_w : h.sg_w) + (long)ai * 256;
          const float* x = h.latent + (long)r * 256;
          float p = 0.f;
          for (int k = 0; k < 256; ++k) p = fmaf(wv[k], x[k], p);
          pre[rl * 2 * A + q] = p + a.P[(q < A ? h.mu_b : h.sg_b) + ai];
        }
        __syncthreads();
        tail_head_rows(h, r0, rows, pre, hsc);
      }
    }
  }
}

static_assert(kCarlaLayers <= kTailMaxLin, "TailArgs holds every layer of the table");

}  // namespace

void launch_carla_pack(const float* vmeas, float* feat, int n, int NV, hipStream_t s) {
  hipLaunchKernelGGL(k_carla_pack, dim3((n * NV + 255) / 256), dim3(256), 0, s, vmeas, feat, n, NV);
}

void launch_carla_head(const HeadArgs& h, hipStream_t s) {
  hipLaunchKernelGGL(k_carla_head, dim3((h.n + 63) / 64), dim3(64), 0, s, h);
}

// The MLP part after conv6's partials (c6, c6_Z) as k_carla_tail: the table's layers in tail order
// (dependency stages, carla_model.h:238-279), then one cooperative launch or one launch per stage.
int launch_carla_tail(const CarlaNet& net, CarlaFwdBufs& fb, const float* P, int n, const ConvArgs& c6, int c6_Z,
                      const float* meas, const float* vmeas, int NM, int NV, float* value, const HeadArgs& h,
                      bool cooperative, hipStream_t s) {
  TailArgs ta{};
  ta.P = P;
  ta.n = n;
  ta.c6 = c6;
  ta.c6_Z = c6_Z;
  ta.vmeas = vmeas;
  ta.feat = fb.feat;
  ta.NV = NV;
  // With a narrow measurement vector the state MLP's first layer runs inside its second layer's
  // items (stage 0, beside conv6's finish): one stage fewer
  const int d = NM <= kTailPreMaxK ? 1 : 0;
  ta.pre_lin = ta.pre_for = -1;
  for (int k = 0; k < kCarlaLayers; ++k) {
    const CarlaLayer& e = net.layer[net.tail_order[k]];
    if (d && e.in == kBufMeas) ta.pre_lin = k;
    if (d && e.in == net.layer[0].out) ta.pre_for = k;
    ta.lin[k] = TailLin{e.in == kBufMeas ? meas : carla_buf(fb, e.in), e.in_stride, e.IN, e.w, e.b,
                        carla_buf(fb, e.out), e.out_stride, e.OUT, e.relu, e.to_value ? value : nullptr};
    ta.lin_stage[k] = e.stage - d;
  }
  ta.nlin = kCarlaLayers;
  ta.nstage = ta.lin_stage[kCarlaLayers - 1] + 1;
  ta.head_stage = ta.nstage - 1;
  ta.h = h;
  ta.bar = fb.tail_bar;
  const int rt_n = (n + 15) / 16;
  const unsigned G = (unsigned)(rt_n * 32);  // linear.0's work items (512 / 16 output tiles)
  if (cooperative) {
    ta.stage_lo = 0;
    ta.stage_hi = ta.nstage - 1;
    ta.bar_base = fb.tail_count;
    void* args[] = {&ta};
    if (hipLaunchCooperativeKernel((const void*)k_carla_tail, dim3(G), dim3(kTailThreads), args, 0, s) != hipSuccess)
      return ppo_fail("ppo_carla_forward: cooperative launch of the fused tail failed", -2);
    fb.tail_count += (unsigned)(ta.nstage - 1) * G;
  } else {
    for (int st = 0; st < ta.nstage; ++st) {
      ta.stage_lo = ta.stage_hi = st;
      hipLaunchKernelGGL(k_carla_tail, dim3(G), dim3(kTailThreads), 0, s, ta);
    }
  }
  if (hipGetLastError() != hipSuccess) return ppo_fail("ppo_carla_forward: launch failed", -2);
  return 0;
}
