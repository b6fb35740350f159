// ppo_carla_internal.hpp — the CaRL agent beyond include/ppo_carla.h, for the units of the library:
//   ppo_carla.hip          the agent: context, layer table, forward, update, I/O, the entry points below
//   ppo_carla_conv.hip     forward convolution kernels (a Linear layer is a 1x1 one), launch_conv
//   ppo_carla_tail.hip     k_carla_pack, k_carla_head, k_carla_tail and their launchers
//   ppo_carla_ln.hip       LayerNorm kernels and launchers, the ppo_carla_debug_ln_* hooks
//   ppo_carla_grad.hip     input- and weight-gradient kernels and launchers
//   ppo_carla_pos.hip      use_positional_encoding: conv1's row / column tables, the two planes' weight gradient
//   ppo_carla_rollout.hip  rollout storage, GAE, the epoch loop, act lanes
// (ppo_carla_units.hpp: what crosses the first six). The rollout object computes through
// ppo_carla_forward / ppo_carla_update and, for its act lanes, carla_forward on a lane's own buffer set;
// the rest reads the agent's placement and moves the statistics that every ppo_carla_update leaves on the
// device, so the epoch loop needs no host synchronisation per minibatch.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/ppo_carla.h"

struct CarlaAgentInfo {
  int device, max_batch;
  hipStream_t stream;  // the agent's own stream (what a NULL stream argument selects)
};
int carla_agent_info(const ppo_carla_t* c, CarlaAgentInfo* out);

// floats per statistics slot: pg_loss, v_loss, entropy, old_approx_kl, approx_kl, clipfrac, grad_norm, (unused)
constexpr int kCarlaStatSlot = 8;
// slot[0..8) = the statistics of the last ppo_carla_update on s (this rank's, not rank-averaged), device to device
int carla_stats_to_slot(ppo_carla_t* c, float* slot, hipStream_t s);

// Everything one forward writes besides its outputs: two forwards may run at the same time exactly when
// each has its own set. The agent is one (its base: the buffers of ppo_carla_forward / ppo_carla_update,
// max_batch rows); an act lane owns another of one row (carla_fwd_alloc).
struct CarlaFwdBufs {
  float* act[PPO_CARLA_NCONV - 1] = {};  // conv1..conv5 outputs
  float *enc = nullptr, *s1 = nullptr, *l1 = nullptr, *feat = nullptr, *v1 = nullptr, *v2 = nullptr, *val = nullptr;
  float *p1 = nullptr, *p2 = nullptr;
  float* hpre = nullptr;    // [B][2A]
  float* ksplit = nullptr;  // split-K partials of the forward's narrow layers (conv_split_z)
  // k_conv_img3's A-operand table: k_conv1_wprep rewrites it from conv1's weights in every forward
  float* c1w = nullptr;
  // positional agents (ppo_carla_create3): conv1's row / column tables [8][OH] | [8][OW], which
  // launch_pos_bias rewrites from conv1's weights in every forward, as c1w is
  float* posb = nullptr;
  unsigned* tail_bar = nullptr;  // k_carla_tail's grid barrier counter
  unsigned tail_count = 0;       // arrivals so far (the counter's value between launches)
  // LayerNorm agents (ppo_carla_create2): per normalised layer the pre-activation z [B][F] and the
  // row statistics {mean, rstd} [B][2]; ln[k].F == 0: the layer has no LayerNorm. g / be: the offsets
  // of gamma / beta in the parameter vector.
  struct Ln {
    int F = 0;
    long g = -1, be = -1;
    float *z = nullptr, *stat = nullptr;
  };
  enum { kLnConv = 0, kLnS1 = 6, kLnS2, kLnL1, kLnFeat, kLnV1, kLnV2, kLnP1, kLnP2, kLnCount };
  Ln ln[kLnCount];
  bool any_ln = false;
};

// ---- the MLP part of the network (carla_model.h:238-279), described once ----
// Its activation buffers by name: a layer names what it reads and writes, so one table serves every buffer
// set and the gradient buffers. kBufMeas is the caller's measurements (in no set); kBufState is columns
// 1024.. of enc (state_linear's output beside conv6's); feat is [256 + NV]: features | value measurements.
enum CarlaBuf { kBufMeas, kBufS1, kBufState, kBufEnc, kBufL1, kBufFeat, kBufV1, kBufV2, kBufVal, kBufP1, kBufP2, kBufCount };
static inline float* carla_buf(const CarlaFwdBufs& fb, int name) {
  float* const p[kBufCount] = {nullptr, fb.s1, fb.enc + 1024, fb.enc, fb.l1, fb.feat, fb.v1, fb.v2, fb.val, fb.p1, fb.p2};
  return p[name];
}
// The gradient of each named buffer (allocated by the first update). d[kBufMeas] and d[kBufState] stay
// null: kBufState's is part of d[kBufEnc]. Rows are as wide as the buffer's, except that d[kBufFeat] has
// no value-measurement columns.
struct CarlaGradBufs {
  float* d[kBufCount] = {};
};
static inline float* carla_grad(const CarlaGradBufs& g, int name) { return name == kBufState ? g.d[kBufEnc] + 1024 : g.d[name]; }
static inline long carla_grad_stride(int name) {
  return name == kBufEnc || name == kBufState ? 1280 : name == kBufL1 ? 512 : name == kBufVal ? 1 : 256;
}
// One Linear layer. CarlaNet (built once by ppo_carla_create2) lists the nine in carla_model.h's forward
// order; buffer sizes, the per-layer forward, the fused tail's arguments and the backward are loops over it.
// The backward is the reverse order, and a layer adds to its input's gradient exactly when a layer after it
// in the forward has stored it (feat, read by both heads); the fused tail runs tail_order, the layers stably
// sorted by stage. dist_mu / dist_sigma are not listed: k_carla_head / k_carla_head_bwd compute them.
struct CarlaLayer {
  int in, out;                 // CarlaBuf
  long in_stride, out_stride;  // floats per row
  int IN, OUT;                 // columns read (value_head.0: 256 + NV of feat, policy_head.0: 256) and written
  long w, b;                   // offsets in the parameter vector
  int relu;
  int ln;        // CarlaFwdBufs::kLn* slot of the LayerNorm after it (used when the slot's F != 0), -1: none
  long g, be;    // that LayerNorm's gamma / beta offsets, -1: none
  int stage;     // fused tail: dependency stage (0: beside conv6's finish)
  bool to_value; // fused tail: column 0 also goes to the caller's `value`
};
constexpr int kCarlaLayers = 9;
struct CarlaNet {
  CarlaLayer layer[kCarlaLayers];
  int tail_order[kCarlaLayers];
};

// a zeroed buffer set of `rows` rows for c's shapes on the current device; -2 if an allocation fails
// (the caller frees what was allocated). The zero fills run on the null stream.
int carla_fwd_alloc(const ppo_carla_t* c, size_t rows, CarlaFwdBufs* fb);
void carla_fwd_free(CarlaFwdBufs* fb);
// ppo_carla_forward's body on buffer set fb (n rows at most what fb was allocated for) and stream s.
// Reads the agent's parameters and options only: forwards on different buffer sets may run from
// different threads at the same time.
int carla_forward(const ppo_carla_t* c, CarlaFwdBufs& fb, hipStream_t s, int n, const uint8_t* bev, const float* meas,
                  const float* vmeas, int sample_type, const float* action_in, long env_base, long step_id,
                  float* action, float* logprob, float* entropy, float* value, float* alpha, float* beta);
// The agent's parameter event: recorded on s after everything queued there so far. ppo_carla_update,
// ppo_carla_load_params and ppo_carla_comm_broadcast_params record it; an act lane's stream waits for it.
int carla_params_mark(ppo_carla_t* c, hipStream_t s);
int carla_params_wait(const ppo_carla_t* c, hipStream_t s);
