// ppo_carla_units.hpp — what crosses the CaRL agent's translation units (listed in
// ppo_carla_internal.hpp): the launchers, their argument blocks and the constants more than one unit needs.
// Kernels stay in each unit's anonymous namespace; the helpers here that kernels of two units share are in
// one too, so every unit compiles its own copy.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/ppo_carla.h"
#include "../../include/ppo_hip.h"
#include "ppo_agent.hpp"
#include "ppo_carla_internal.hpp"
#include "ppo_kernels.hpp"

struct ConvArgs {
  const float* in_f;
  const uint8_t* in_u8;
  long in_stride;  // elements per sample
  int IC, IH, IW;
  const float* W;  // [OC][IC * K * K]
  const float* b;
  float* out;
  long out_stride;  // elements per sample
  int OC, OH, OW;
  int K, S, relu;
  int n;
  float* part;  // split-K partial sums [Z][n * OH * OW][OC] (launch_conv sets kc and part)
  int kc;       // k-range per blockIdx.z (0: no split)
  float* wprep = nullptr;  // conv1 packed form (k_conv_img3): its A operands, [kImg3Blocks][4][16][4]
  int bx = 0;              // conv1 packed form: 1 runs its products as split-bf16 MFMAs (k_conv_img3<.., BX>)
  int tiled = 0;           // 1: conv2's shape runs k_conv_t (LDS-staged input patches)
  // uint8 input only (conv1). wstride: floats between two filters of W (0: IC * K * K; a positional
  // agent's cnn.0.weight is [OC][IC + 2][K][K], of which the image channels are the first IC * K * K).
  // xscale: what a byte is multiplied by (1 / 255; 1 for a positional agent, carla_model.h:222-236).
  // rowb [OC][OH] / colb [OC][OW]: the two coordinate planes' part of the pre-activation
  // (launch_pos_bias), added with the bias; null: none.
  int wstride = 0;
  float xscale = 1.0f / 255.0f;
  const float* rowb = nullptr;
  const float* colb = nullptr;
};

constexpr int kMaxKTab = 2048;  // im2col offset table entries (IC * K * K <= 1280 here)
constexpr int kUK = 4;          // k-steps per loop iteration: their loads are all in flight together

constexpr int kConv1Auto = 2;  // the default conv1 form (ppo_carla_create_ex option conv1): packed (measured faster)
// conv1_mfma=auto: the split-bf16 form (bx3). cfg5's 2 048-row update 12.33 -> 10.63 ms, batch-256
// forward 0.69 -> 0.58 ms (profiles/r05/carla_bx/); gradient vs the fp32 torch reference 6.7e-7 rel-L2
// (test_conv1_split_bf16_update_vs_torch)
constexpr int kConv1BxAuto = 1;
// conv_dgrad=auto: the quad form (k_dgrad_q, one GEMM over the four parity classes)
constexpr int kDgradQuadAuto = 1;
// conv_wgrad=auto: the LDS-tiled form (k_wgrad_t)
constexpr int kWgradTiledAuto = 1;
// conv_fwd=auto: the LDS-tiled form (k_conv_t)
constexpr int kConvTiledAuto = 1;
// deep_dgrad=auto: conv6's input gradient as a dense GEMM + col2im
constexpr int kDgradColAuto = 1;

struct HeadArgs {
  const float* P;
  long mu_w, mu_b, sg_w, sg_b, hi, lo;
  const float* latent;  // [n][256] policy_head output
  const float* val;     // [n]
  int n, A, mode;
  float beta_min;
  const float* action_in;
  uint64_t seed;
  int rank;
  long env_base, step_id;
  float *action, *logprob, *entropy, *value, *alpha, *beta;
  float* hpre;  // [n][2A] dist_mu / dist_sigma pre-activations (training), may be null
};

struct DgradArgs {
  const float* dz;  // [n][OC][OH*OW], sample stride dz_stride
  long dz_stride;
  const float* W;   // W[oc][w_ic][K][K]
  int w_ic;
  const float* x;   // the layer input (post-ReLU) for the mask, [n][IC][IH*IW]
  long x_stride;
  float* dx;
  long dx_stride;
  int IC, IH, IW, OC, OH, OW, K, S, n, accumulate;
};

struct WgradArgs {
  const float* dz;  // [n][OC][OP], sample stride dz_stride
  long dz_stride;
  int OC, OP, OW;
  const float* x_f;
  const uint8_t* x_u8;
  long x_stride;
  int IC, IH, IW, K, S;
  int n, Kt;     // Kt = IC*K*K; column Kt is the bias (x = 1)
  long qchunk;   // output pixels per chunk (multiple of 4)
  float* part;   // [chunks][OC][Kt + 1]
  long group_bytes = 0;  // host only: launch_wgrad_generic's sample-group limit (0: kWgradFar)
  int wstride = 0;       // floats between two filters of Gw (0: Kt), as ConvArgs::wstride
  float xscale = 1.0f / 255.0f;  // uint8 input: what a byte is multiplied by, as ConvArgs::xscale
};

struct WgradPlan {
  int not_, ocg, kg, chunks;
  long qchunk;
  size_t part_floats;
};

constexpr int kTailMaxN = 64;  // rows up to which the MLP part runs as k_carla_tail

namespace {

// split-K policy, by layer shape only (so every output element sums its k range in the same
// chunks for any batch): few output pixels per sample and a deep reduction — the Linear layers,
// conv5 and conv6 — get 128-wide k chunks. With few rows (the rollout's batches) those layers
// otherwise run a handful of workgroups whose waves each walk the whole reduction as one
// latency-bound load chain.
constexpr int kSplitKC = 128;
inline int conv_split_z(int Kt, int P) { return (P <= 16 && Kt >= 256) ? (Kt + kSplitKC - 1) / kSplitKC : 1; }

constexpr int kImgTile = 16;
template <int K, int S>
struct ImgGeo {
  static constexpr int TI = (kImgTile - 1) * S + K;  // input patch edge
  static constexpr int TIP = (TI + 3) & ~3;          // patch row pitch in bytes (whole dwords)
};

// 16-tap A blocks of the packed table (two kernel rows each), rounded up to an even count: the BX loop
// reads blocks in pairs (2 kk, 2 kk + 1), so an odd IC * K / 2 (e.g. obs_num_channels 1, 5, 9, 13) gets
// a zero block (k_conv1_wprep writes 0 for rows past IC * K; a zero weight adds exactly 0)
__host__ __device__ inline int img3_blocks(int IC, int K) { return (((IC * K + 1) / 2) + 1) & ~1; }

// conv6 only: for conv5 (stride 2, 10 x 10 -> 4 x 4) the col2im pass costs more than the GEMM saves
// (GEMM 77 + col2im 127 us vs k_dgrad's 182 us; conv6: 5 + 71 + 33 vs 370 us; profiles/r05/carla_tiled/)
// torch.linspace(-1, 1, n)[i] in fp32, bit for bit (ATen's RangeFactories: step = (end - start) / (n - 1),
// the first half counts up from the start and the rest down from the end, each one fused multiply-add)
__host__ __device__ inline float pos_lin(int i, int n) {
  if (n <= 1) return -1.0f;
  const float step = (1.0f - (-1.0f)) / (float)(n - 1);
  return i < n / 2 ? fmaf(step, (float)i, -1.0f) : fmaf(-step, (float)(n - 1 - i), 1.0f);
}
constexpr int kPosMaxOW = 256;  // k_pos_rq keeps a lane's column sums in four registers (64 lanes x 4)
constexpr int kPosMaxOH = 1024; // and a workgroup's row sums in LDS
constexpr int kPosSPC = 4;      // samples per workgroup of k_pos_rq: its partial count depends on n only

inline bool dgrad_col_layer(int OH, int OW, int K = 3, int S = 1) { return OH * OW <= 16 && K == 3 && S == 1; }

}  // namespace

// hidden: the library's exported symbols stay those of the C ABI and ppo_carla_internal.hpp
#pragma GCC visibility push(hidden)
// ppo_carla_conv.hip. fin = false: a split-K layer leaves its partials (k_conv_fin is the caller's, e.g.
// the fused tail's stage 0); *z_out receives the chunk count (1: not split)
int launch_conv(const ConvArgs& a, hipStream_t s, int img = 1, bool fin = true, int* z_out = nullptr);
// ppo_carla_tail.hip
void launch_carla_pack(const float* vmeas, float* feat, int n, int NV, hipStream_t s);
void launch_carla_head(const HeadArgs& h, hipStream_t s);
int launch_carla_tail(const CarlaNet& net, CarlaFwdBufs& fb, const float* P, int n, const ConvArgs& c6, int c6_Z,
                      const float* meas, const float* vmeas, int NM, int NV, float* value, const HeadArgs& h,
                      bool cooperative, hipStream_t s);
// ppo_carla_ln.hip
size_t ln_part_floats(int max_n, int F);
void launch_ln_fwd(int n, int F, const float* z, long zs, const float* gamma, const float* beta, float* y, long ys,
                   float* stat, hipStream_t s);
int launch_ln_bwd(int n, int F, float* d, long ds, const float* z, long zs, const float* gamma, const float* stat,
                  float* dgamma, float* dbeta, float* part, size_t part_cap, hipStream_t s);
// ppo_carla_grad.hip
int launch_dgrad(const DgradArgs& a, hipStream_t s, bool staged = true, bool quad = false);
int launch_dgrad_col(const DgradArgs& a, float* wt, const float* zbias, float* dcol, hipStream_t s);
WgradPlan plan_wgrad(int OC, int Kt, long Q);
int launch_wgrad(WgradArgs a, float* Gw, float* Gb, float* part, size_t part_cap, hipStream_t s, bool img = true,
                 bool bx = false, bool tiled = false);
// ppo_carla_pos.hip: use_positional_encoding's two constant input planes, never materialised.
// rowb [OC][OH], colb [OC][OW] from W [OC][IC_total][K][K] (planes C and C + 1)
int launch_pos_bias(int OC, int IC_total, int C, int K, int S, int IH, int IW, const float* W, float* rowb,
                    float* colb, hipStream_t s);
// floats of the row / column partial sums for up to max_n samples
size_t pos_part_floats(int max_n, int OC, int OH, int OW);
// dw [oc * dw_stride + {0, 1} * K * K + ky * K + kx] from dz [n][OC][OH][OW] (sample stride dz_stride)
int launch_pos_wgrad(int n, int OC, int OH, int OW, int K, int S, int IH, int IW, const float* dz, long dz_stride,
                     float* dw, long dw_stride, float* part, size_t part_cap, hipStream_t s);
#pragma GCC visibility pop
