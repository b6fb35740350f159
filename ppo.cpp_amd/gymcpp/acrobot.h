// gymcpp/acrobot.h — AcrobotContinuous-v1 behind the Environment interface: Gymnasium's Acrobot-v1
// ("book" dynamics, one RK4 step of 0.2 s per env step) with the torque clip(a, -1, 1) from one
// continuous action (O = 6, A = 1, action space [-1, 1], reward -1 per step and 0 on the terminating
// one, termination when the tip swings above the bar, 500-step truncation). The arithmetic is
// include/ppo_acrobot.h, shared with the device env (include/ppo_synth_env.h, PSYN_ACROBOT), so host
// and device trajectories are bit-identical (compile with -ffp-contract=off). Reset noise as
// Pendulum's: Philox4x32-10 keyed (seed, 0x5EED5EED), counter (resets, i), i = 0..3 for theta1,
// theta2, theta1dot, theta2dot.
#pragma once

#include <cstdint>

#include "../../include/ppo_acrobot.h"
#include "gym.h"
#include "synthetic_cheetah.h"  // philox4x32_host

namespace gymcpp {

class AcrobotContinuous final : public Environment {
  float s_[ACRO_STATE_DIM] = {0.0f, 0.0f, 0.0f, 0.0f};
  float obs_[ACRO_OBS_DIM] = {1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};
  uint32_t rseed_ = 1, rcount_ = 0;
  int elapsed_ = ACRO_MAX_STEPS + 1;

 public:
  // seed > 0 re-keys the reset noise; otherwise the reset count continues
  ObsView reset(int seed) override {
    if (seed > 0) { rseed_ = (uint32_t)seed; rcount_ = 0; }
    float u[ACRO_STATE_DIM];
    for (int i = 0; i < ACRO_STATE_DIM; ++i) {
      uint32_t r[4];
      philox4x32_host(rcount_, (uint32_t)i, 0u, 0u, rseed_, 0x5EED5EEDu, r);
      u[i] = ((float)(r[0] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    }
    acro_reset(u, s_);
    (void)acro_obs(s_, obs_);
    rcount_ += 1;
    elapsed_ = 0;
    return ObsView{obs_, ACRO_OBS_DIM};
  }
  std::tuple<ObsView, float, bool, bool> step(const float* a) override {
    float term = 0.0f;
    const float reward = acro_step(s_, a[0], obs_, &term);
    ++elapsed_;
    return {ObsView{obs_, ACRO_OBS_DIM}, reward, term != 0.0f, elapsed_ >= ACRO_MAX_STEPS};
  }
  int get_observation_space() const override { return ACRO_OBS_DIM; }
  int get_action_space() const override { return ACRO_ACT_DIM; }
  float get_action_space_min() const override { return -1.0f; }
  float get_action_space_max() const override { return 1.0f; }
  const float* state() const { return s_; }
  void set_state(const float* s) {
    for (int i = 0; i < ACRO_STATE_DIM; ++i) s_[i] = s[i];
    (void)acro_obs(s_, obs_);
    elapsed_ = 0;
  }
};

}  // namespace gymcpp
