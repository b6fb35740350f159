// ppo_carla_internal.hpp — what ppo_carla_rollout.hip needs from the agent beyond include/ppo_carla.h
// (defined at the end of ppo_carla.hip). The rollout object computes through ppo_carla_forward /
// ppo_carla_update and, for its act lanes, carla_forward on a lane's own buffer set; the rest reads the
// agent's placement and moves the statistics that every ppo_carla_update leaves on the device, so the
// epoch loop needs no host synchronisation per minibatch.
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
