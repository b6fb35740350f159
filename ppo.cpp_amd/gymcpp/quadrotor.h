// gymcpp/quadrotor.h — QuadrotorHover-v0 behind the Environment interface: a rigid-body quadrotor in
// "+" configuration hovering at the origin (O = 18, A = 4, action space [-1, 1]^4, termination when
// |p|^2 > 9, 500-step truncation). It is this project's own task over the textbook Newton-Euler
// equations, not a simulator's quadrotor. The arithmetic is include/ppo_quadrotor.h, shared with the
// device env (include/ppo_synth_env.h, PSYN_QUADROTOR), so host and device trajectories are
// bit-identical (compile with -ffp-contract=off). Reset noise as Pendulum's: Philox4x32-10 keyed
// (seed, 0x5EED5EED), counter (resets, i), i = 0..11 for p, v, the quaternion's vector part and omega.
#pragma once

#include <cstdint>

#include "../../include/ppo_quadrotor.h"
#include "gym.h"
#include "synthetic_cheetah.h"  // philox4x32_host

namespace gymcpp {

class QuadrotorHover final : public Environment {
  float s_[QUAD_STATE_DIM] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float obs_[QUAD_OBS_DIM] = {};
  uint32_t rseed_ = 1, rcount_ = 0;
  int elapsed_ = QUAD_MAX_STEPS + 1;

 public:
  // seed > 0 re-keys the reset noise; otherwise the reset count continues
  ObsView reset(int seed) override {
    if (seed > 0) { rseed_ = (uint32_t)seed; rcount_ = 0; }
    float u[QUAD_RESET_DRAWS];
    for (int i = 0; i < QUAD_RESET_DRAWS; ++i) {
      uint32_t r[4];
      philox4x32_host(rcount_, (uint32_t)i, 0u, 0u, rseed_, 0x5EED5EEDu, r);
      u[i] = ((float)(r[0] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    }
    quad_reset(u, s_);
    quad_obs(s_, obs_);
    rcount_ += 1;
    elapsed_ = 0;
    return ObsView{obs_, QUAD_OBS_DIM};
  }
  std::tuple<ObsView, float, bool, bool> step(const float* a) override {
    float term = 0.0f;
    const float reward = quad_step(s_, a, obs_, &term);
    ++elapsed_;
    return {ObsView{obs_, QUAD_OBS_DIM}, reward, term != 0.0f, elapsed_ >= QUAD_MAX_STEPS};
  }
  int get_observation_space() const override { return QUAD_OBS_DIM; }
  int get_action_space() const override { return QUAD_ACT_DIM; }
  float get_action_space_min() const override { return -1.0f; }
  float get_action_space_max() const override { return 1.0f; }
  const float* state() const { return s_; }
  void set_state(const float* s) {
    for (int i = 0; i < QUAD_STATE_DIM; ++i) s_[i] = s[i];
    elapsed_ = 0;
  }
};

}  // namespace gymcpp
