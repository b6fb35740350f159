// gymcpp/reacher.h — ReacherPlanar-v0 behind the Environment interface: a two-link planar arm with
// Gymnasium Reacher-v5's task definition (observation layout, reward, goal distribution, 50-step
// truncation, action space [-1, 1]^2; O = 10, A = 2; never terminates) over the textbook two-link
// manipulator equations. It is not MuJoCo's Reacher. The arithmetic is include/ppo_reacher.h, shared
// with the device env (include/ppo_synth_env.h, PSYN_REACHER), so host and device trajectories are
// bit-identical (compile with -ffp-contract=off). Reset noise as Pendulum's: Philox4x32-10 keyed
// (seed, 0x5EED5EED), counter (resets, i), i = 0..5 for q1, q2, q1dot, q2dot and the goal's radius
// and angle. The goal is part of the state: a step never changes it, every reset draws a new one.
#pragma once

#include <cstdint>

#include "../../include/ppo_reacher.h"
#include "gym.h"
#include "synthetic_cheetah.h"  // philox4x32_host

namespace gymcpp {

class ReacherPlanar final : public Environment {
  float s_[REACH_STATE_DIM] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float obs_[REACH_OBS_DIM] = {};
  uint32_t rseed_ = 1, rcount_ = 0;
  int elapsed_ = REACH_MAX_STEPS + 1;

 public:
  // seed > 0 re-keys the reset noise; otherwise the reset count continues
  ObsView reset(int seed) override {
    if (seed > 0) { rseed_ = (uint32_t)seed; rcount_ = 0; }
    float u[REACH_STATE_DIM];
    for (int i = 0; i < REACH_STATE_DIM; ++i) {
      uint32_t r[4];
      philox4x32_host(rcount_, (uint32_t)i, 0u, 0u, rseed_, 0x5EED5EEDu, r);
      u[i] = ((float)(r[0] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    }
    reach_reset(u, s_);
    reach_obs(s_, obs_);
    rcount_ += 1;
    elapsed_ = 0;
    return ObsView{obs_, REACH_OBS_DIM};
  }
  std::tuple<ObsView, float, bool, bool> step(const float* a) override {
    const float reward = reach_step(s_, a, obs_);
    ++elapsed_;
    return {ObsView{obs_, REACH_OBS_DIM}, reward, false, elapsed_ >= REACH_MAX_STEPS};
  }
  int get_observation_space() const override { return REACH_OBS_DIM; }
  int get_action_space() const override { return REACH_ACT_DIM; }
  float get_action_space_min() const override { return -1.0f; }
  float get_action_space_max() const override { return 1.0f; }
  const float* state() const { return s_; }
  void set_state(const float* s) {
    for (int i = 0; i < REACH_STATE_DIM; ++i) s_[i] = s[i];
    elapsed_ = 0;
  }
};

}  // namespace gymcpp
