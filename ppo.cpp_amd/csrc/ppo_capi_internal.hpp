// ppo_capi_internal.hpp — what the C-ABI's translation units share: the context (ppo_ctx), the kernel
// plan made at create (KernelPlan, ppo_capi_plan.hip), the update's prebuilt kernel arguments
// (UpdatePlan, ppo_capi_update.hip), the device env and wrapper handles, the error / profiling helpers.
//
//   ppo_capi.hip         errors, runtime check, obs-norm, create / destroy, parameter and Adam I/O, act,
//                        values, GAE, snapshots, device helpers, kernel_info, profiling
//   ppo_capi_plan.hip    the create options, their auto constants, the kernel planner
//   ppo_capi_update.hip  ppo_update / ppo_update_ex
//   ppo_capi_comm.hip    the communicator (RCCL or the host transport) and the all-reduce
//   ppo_capi_env.hip     the device env, its wrapper chain, the device-resident rollout and evaluation
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ppo_hip.h"
#include "../../include/ppo_synth_env.h"
#include "../../include/ppo_env_wrappers.h"
#include "ppo_kernels.hpp"

// ------------------------------------------------------------------------------------------
// errors: one thread_local message (ppo_capi.hip), set through ppo_fail
// ------------------------------------------------------------------------------------------
static inline int fail(const std::string& msg, int code = -1) { return ppo_fail(msg, code); }
#define HIP_TRY(expr)                                                                           \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_), -2);   \
  } while (0)
#define NCCL_TRY(expr)                                                                          \
  do {                                                                                          \
    ncclResult_t r_ = (expr);                                                                   \
    if (r_ != ncclSuccess) return fail(std::string(#expr) + ": " + ncclGetErrorString(r_), -3); \
  } while (0)

template <typename T>
static int dmalloc(T** p, size_t n) {
  if (n == 0) n = 1;
  hipError_t e = hipMalloc((void**)p, n * sizeof(T));
  if (e != hipSuccess) return fail(std::string("hipMalloc: ") + hipGetErrorString(e), -2);
  (void)hipMemset(*p, 0, n * sizeof(T));
  return 0;
}

// ------------------------------------------------------------------------------------------
// the kernel plan: every selection ppo_create_ex makes, decided by plan_kernels (ppo_capi_plan.hip)
// from the config and the options before anything is allocated. The allocations are sized from it,
// the launch sequences read it, ppo_kernel_info prints its names.
// ------------------------------------------------------------------------------------------
struct KernelPlan {
  int tiles_per_block = 1, nblk = 1;  // k_fwdbwd's grid over the 64-row tiles of a minibatch
  bool use_upd = false;  // feature-split k_upd (ppo_update.hip) instead of k_fwdbwd
  bool use_upd32 = false;  // k_upd32 (32x32x2 MFMAs) instead of k_upd (create option upd_mfma)
  int upd_bx = 0;          // 1: k_upd's 256-wide GEMMs as split-bf16 piece products (upd_mfma=bx6); 2: k_upd2's layer 1
  int gae_scan = -1;       // 1: GAE as k_gae_scan (create option gae=scan); 0: the bit-exact serial k_gae; -1 auto
  int gae_scan_min_t = 0;  // gae=auto: k_gae_scan from this many collected steps on (kGaeScanMinT)
  // 1: the rollout's critic pass is k_vbx (layer 2 as split-bf16 products; create option values_mfma),
  // run once over the stored rows: the per-step act kernels skip the critic and leave it pending
  int values_bx = 0;
  // the minibatch's k_upd + dW in msplit launch pairs of Mq rows each (create option upd_split): the
  // hand-off rows (H1 / DZ1 / DZ2 / Xn) of one pair are ~M / msplit x 6 KB, small enough to stay in the
  // 256 MB Infinity Cache between k_upd's stores and k_dwf's reads
  int msplit = 1, Mq = 0;
  // 1: k_upd writes no H1 rows, only each row's layer-1 LayerNorm (mean, 1 / std) into LNS[trunk]
  // ([M][2]), and k_dwf_bx recomputes H1 bitwise (create option h1_handoff)
  int h1_recomp = 0;
  int upd32_mix = 0;       // k_upd32 with the actor trunk on k_upd's body (upd_mfma=mix)
  bool use_upd2 = false;  // two-trunk k_upd2 (ppo_update_narrow.hip, H = 64 tanh agent)
  int rollout_kernel = 0;   // AC persistent rollout: 0 auto, 1 k_rollout (MFMA), 2 k_rollout_v (VALU), 3 k_rollout_s
  int upd2_split = 0;       // k_l1g (layer 1 as a gathered GEMM into Z1) + k_upd2's split form at 2 / 3 per CU
  UpdGeoOut upd = {};       // LDS geometry of the chosen k_upd / k_upd32 / k_upd2 form
  int upd_nblk = 0;         // its workgroups per trunk
  size_t lds_bytes = 0;     // k_fwdbwd's LDS
  int wlds_off = 0;
  int nchunks = 1, rows_per_chunk = 64, dw_slices = 1;  // dW split-K geometry (of one Mq-row launch pair)
  int gn_fold = 0;                      // create option gradnorm: 1 fold the norm slices into k_colsum
  int act_kernel = 0;  // 0: the fastest act kernel for the shape; 2 / 4: force k_act2 / k_act4 (PPO_ACT_KERNEL, A/B)
  int upd_trunk_mask = 3, upd_sched = 1;   // k_upd launch options (PPO_UPD_TRUNK: PPO_DIAG builds only)
  int upd_hot = 0;                      // PPO_UPD2_HOT (PPO_DIAG builds only): UpdArgs::hot
  int dw_fused = 1;
  bool no_update = false;               // create option update=off: no update kernel is prepared, ppo_update refuses
  int dw_dma = 1;                       // create option dw_dma: k_dwf stages by LDS DMA (k_dwf_dma)
  int dw_bx = 0;                        // create option dw_mfma: 0 fp32 MFMA, 8 / 9 exact bf16 piece products (k_dwf_bx)
  int dw_so = 0;                        // create option dw_stage: k_dwf_bx's split-once form (k_dwf_so)
  int gradstep = 0;                     // create option gradstep=fused|split (default split)
  int update_graph = 0;                 // create option update_graph: replay the minibatch loop as a hipGraph
  bool update_graph_auto = false;       // ... chosen by update_graph=auto (then off once snapshots are taken)
  // what ppo_kernel_info prints: update= dw= values= norm= and, for the opt-in rollout kernel, rollout=
  std::string upd_name, dw_name, values_name, norm_name, rollout_name;
};

// Kernel selection options of ppo_create_ex: "key=value" pairs separated by ',' (include/ppo_hip.h).
// What each auto stands for is with the planner (ppo_capi_plan.hip).
struct CreateOptions {
  int upd_kernel = 0;   // 0 auto, 1 the wave-per-16-rows k_fwdbwd
  int act_kernel = 0;   // 0 auto, 2 / 4 force k_act2 / k_act4
  int dw_fused = 1;
  // update=off: a context that acts and evaluates only. ppo_create does not size the fused update
  // kernel's LDS, whose 2 A head rows pass 160 KB from A = 13 on at hidden 256 (the refusal of
  // the default), so the AC agent exists at Humanoid's A = 17; ppo_update refuses.
  int update = 1;
  int rollout = PPO_ROLLOUT_AUTO;
  // 1: grad norm + Adam in one cooperative launch (k_gradstep); 0 (default): two launches. A
  // cooperative launch costs ~30 us on this stack (measured: cfg1 +8.5 ms per iteration), more
  // than the launch it saves.
  int gradstep = 0;
  int gradnorm = -1;   // gradnorm=auto|slices|fold: clip_grad_norm_'s sums of squares by k_gradnorm or inside k_colsum
  int dw_rows = 0;     // dW split-K rows per chunk (multiple of 16; 0: auto, ~128 chunks per trunk)
  int dw_slices = 0;   // k_dwf output slices per chunk (1 / 2; 0: auto, dw_slices())
  int dw_dma = 1;      // 1 (default): k_dwf_dma (LDS-DMA staging, three stage buffers); 0: k_dwf
  int dw_bx = -1;      // dw_mfma: -1 auto, 0 f32 (fp32 MFMA), 9 / 8 / 6 bf16x9 / x8 / x6 (k_dwf_bx: exact bf16 splits)
  int gae_scan = -1;   // gae=auto (scan from kGaeScanMinT steps) | serial (bit-exact with the reference's loop) | scan
  int values_mfma = -1;  // values_mfma=auto (bx6 where k_upd's bx6 pieces exist) | f32 | bx6
  int upd_split = 0;     // upd_split=auto|1|2|4|8: minibatch rows per k_upd + dW launch pair (M / n)
  int h1_handoff = -1;   // h1_handoff=auto|store|recompute: H1 rows from k_upd, or recomputed by k_dwf_bx
  int dw_stage = -1;     // dw_stage=auto|dma|split_once: k_dwf_bx (LDS-DMA stages, split per consumer) or k_dwf_so
  // 1: ppo_update replays its minibatch launches as one captured hipGraph; 0: eager. auto stays eager
  // from the first ppo_snapshot_state on (a thread that reads snapshots while the owner captures made
  // the capture fail); 1 keeps the graph with snapshots, for callers that use the context from one thread.
  int update_graph = -1;  // -1 auto (kUpdGraphAutoRows), 0 eager, 1 graph
  int rollout_kernel = 0;  // 0 auto, 1 mfma (k_rollout), 2 valu (k_rollout_v), 3 split (k_rollout_s)
  int upd2_split = -1;  // -1 auto (= kUpd2SplitAuto: the single k_upd2), 0 one k_upd2, 2 / 3 split at 2 / 3 workgroups per CU
  int upd_mfma = 0;     // 0 auto (bx6 where it applies, else 16), 16: k_upd (16x16x4 fp32 MFMAs),
                        // 32: k_upd32 (32x32x2; LayerNorm-Beta agent, H = 256),
                        // 1: k_upd32's mixed form (critic 32x32x2, actor 16x16x4),
                        // 6: bx6, k_upd with its 256-wide GEMMs as split-bf16 piece products (k_upd<.., BX>)
};
int parse_create_options(const char* opts, CreateOptions* o);  // ppo_capi_plan.hip
// Fills the plan, or refuses through fail(). Runs after hipSetDevice (the *_supported functions set their
// kernels' LDS attribute) and allocates nothing.
int plan_kernels(const ppo_hip_config& cfg, const PackedLayout& K, const SmallGradLayout (&sg)[2], const CreateOptions& opt,
                 KernelPlan* plan);

// ------------------------------------------------------------------------------------------
// the update's kernel arguments, built once at the end of create (build_update_plan,
// ppo_capi_update.hip) from the context and the kernel plan. ppo_update_ex copies it and sets what
// varies per call (the permutation, the communicator's world, lr) or per minibatch.
// ------------------------------------------------------------------------------------------
struct UpdatePlan {
  AdvArgs aa;
  UpdArgs u;
  DwArgs dw;
  ColsumArgs cs;
  int ns = 0;           // column-sum segments: the gradient's, then three statistics of the minibatch
  long maxlen = 0;
  int stats_seg0 = 0;   // first of the three
  NormArgs na;
  AdamArgs ad;
  int tb = -1;          // packed offset of the first trainable tensor
  long trainable_n = 0;
  int nblk = 0;         // workgroups that write a slab row (per launch)
  int nsrow = 0;        // slab rows of one minibatch (msplit launches)
  // gradnorm=fold as far as create can tell: every norm tensor is exactly one gradient segment of the
  // column sums. An attached communicator still turns it off (its all-reduce changes the gradient
  // between the column sums and the norm)
  bool fold_ok = false;
};

// ------------------------------------------------------------------------------------------
// profiling (HIP events around the context's launches)
// ------------------------------------------------------------------------------------------
enum {
  PK_ACT = 0, PK_FWDBWD, PK_DW2, PK_DW1, PK_COLSUM, PK_GRADNORM, PK_ADAM, PK_GAE, PK_PERM, PK_ADV, PK_ALLREDUCE,
  PK_SYNTH, PK_ROLLOUT, PK_VALUES, PK_L1G, PK_COUNT
};

struct ProfEvent {
  int id;
  hipEvent_t a, b;
};

struct ppo_ctx {
  ppo_hip_config cfg;
  int device = 0;
  hipStream_t stream = nullptr;
  ppo_layout L;
  PackedLayout K;
  SmallGradLayout sg[2];
  long B = 0;
  int M = 0, nmb = 0;
  KernelPlan plan;
  UpdatePlan up;
  float *P = nullptr, *G = nullptr, *Am = nullptr, *Av = nullptr, *W2T[2] = {nullptr, nullptr};
  float* WSW[2] = {nullptr, nullptr};  // swizzled W1 | W2 | W2^T per trunk (sw_index)
  float* buf[PPO_BUF_COUNT] = {};
  float* next_value = nullptr;
  int32_t* perms = nullptr;
  float *advstats = nullptr, *advsq = nullptr;
  double* advpart = nullptr;
  float *Xn = nullptr, *H1[2] = {}, *DZ1[2] = {}, *DZ2[2] = {};
  float* slab[2] = {};
  std::atomic<int> values_pending{0};  // steps [0, n) of the rollout storage whose values are not computed yet
  float* LNS[2] = {nullptr, nullptr};  // plan.h1_recomp: each row's layer-1 LayerNorm (mean, 1 / std)
  float* Z1 = nullptr;      // plan.upd2_split: [Mr][128] layer-1 pre-activations of the minibatch
  float* dwslab[4] = {};
  float* normout = nullptr;
  float* gnpart = nullptr;
  float* cs_sq = nullptr;               // gradnorm=fold: k_colsum's per-tile sums of squares
  unsigned* cs_cnt = nullptr;           // ... and its per-segment arrival counters (reset by each last arriver)
  float* mbstats = nullptr;  // [EP*MB][8]
  float* snap = nullptr;     // ppo_snapshot_state: P | Am | Av (packed)
  hipEvent_t snap_ev = nullptr;
  hipStream_t snap_stream = nullptr;
  long snap_step = 0;
  long adam_step = 0;
  long iteration = 0;
  ncclComm_t comm = nullptr;
  ppo_host_allreduce_fn host_ar = nullptr;  // host transport (ppo_comm_init_host)
  void* host_user = nullptr;
  std::vector<float> host_stage;
  int world = 1, rank = 0;  // data-parallel group of the attached communicator (1 / cfg.rank without one)
  int rollout_mode = PPO_ROLLOUT_AUTO;  // create option rollout, ppo_set_rollout_mode
  unsigned* gs_bar = nullptr;           // k_gradstep's grid barrier counter
  unsigned gs_count = 0;                // its arrivals so far
  hipGraphExec_t upd_exec = nullptr;    // the captured minibatch loop (all epochs x minibatches)
  const int32_t* upd_exec_perms = nullptr;
  long upd_calls = 0;
  float* sched = nullptr;               // per-minibatch (step size, sqrt(bc2)), AdamArgs::sched
  float* sched_host[2] = {};            // pinned staging of that table, alternating per replay
  hipEvent_t sched_ev[2] = {};          // the H2D copy out of sched_host[i] has completed
  int sched_flip = 0;
  float* beta_store = nullptr;          // persistent AC rollout: (alpha, beta, sample) per (t, env, action)
  int rollout_path = 0;                 // last ppo_rollout_synth: 0 none yet, 1 k_rollout (or _v / _s), 2 per-step launches, 3 k_rollout4, 4 k_rollout_w
  int eval_path = 0;                    // last ppo_evaluate_synth: 0 none yet, 1 k_eval, 2 per-step launches, 3 k_eval4, 4 k_eval_w
  // profiling
  unsigned prof_mask = 0;
  std::mutex prof_mu;
  std::vector<ProfEvent> pending;
  std::vector<hipEvent_t> free_events;
  double prof_ms[PK_COUNT] = {};
  long prof_cnt[PK_COUNT] = {};
};

static inline hipEvent_t prof_event(ppo_t* c) {
  if (!c->free_events.empty()) {
    hipEvent_t e = c->free_events.back();
    c->free_events.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}
struct ProfScope {
  ppo_t* c;
  int id;
  hipStream_t s;
  hipEvent_t a = nullptr, b = nullptr;
  ProfScope(ppo_t* c_, int id_, hipStream_t s_) : c(c_), id(id_), s(s_) {
    if (c->prof_mask & (1u << id)) {
      std::lock_guard<std::mutex> lk(c->prof_mu);
      a = prof_event(c);
      b = prof_event(c);
      (void)hipEventRecord(a, s);
    }
  }
  ~ProfScope() {
    if (a) {
      (void)hipEventRecord(b, s);
      std::lock_guard<std::mutex> lk(c->prof_mu);
      c->pending.push_back({id, a, b});
    }
  }
};

static inline hipStream_t S(ppo_t* c, void* s) { return s ? (hipStream_t)s : c->stream; }
static inline bool distributed(const ppo_t* c) { return c->comm != nullptr || c->host_ar != nullptr; }

// ------------------------------------------------------------------------------------------
// shared between the translation units
// ------------------------------------------------------------------------------------------
void build_update_plan(ppo_t* c);                                                  // ppo_capi_update.hip
int allreduce(ppo_t* c, float* buf, long n, int average, hipStream_t s);           // ppo_capi_comm.hip
void comm_detach(ppo_t* c);
int refresh_weight_copies(ppo_t* c);                                               // ppo_capi.hip
int run_values(ppo_t* c, const float* obs, float* values, long n, hipStream_t s);
int flush_values(ppo_t* c, hipStream_t s);

// ------------------------------------------------------------------------------------------
// device env handles (ppo_capi_env.hip)
// ------------------------------------------------------------------------------------------
struct psyn_env {
  SynthArgs a;
  float act_lo = -1.0f, act_hi = 1.0f;  // the env's action space (clip_actions, gym.h:141-144)
  int device;
  float* host_stats = nullptr;  // pinned [3][E]: psyn_episode_stats_begin / _end
  hipEvent_t stats_ev = nullptr;
};

struct pwrap {
  WrapArgs w;
  int E, O;
  float* state = nullptr;  // 2*E*O + 5*E floats (orc_vwrap_* layout)
};
