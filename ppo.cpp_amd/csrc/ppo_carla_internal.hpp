// ppo_carla_internal.hpp — what ppo_carla_rollout.hip needs from the agent beyond include/ppo_carla.h
// (defined at the end of ppo_carla.hip). The rollout object computes through ppo_carla_forward /
// ppo_carla_update only; these read the agent's placement and move the statistics that every
// ppo_carla_update leaves on the device, so the epoch loop needs no host synchronisation per minibatch.
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
