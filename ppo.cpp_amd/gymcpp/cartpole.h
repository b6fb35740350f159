// gymcpp/cartpole.h — CartPoleContinuous-v1 behind the Environment interface: Gymnasium's CartPole-v1
// with the force force_mag * clip(a, -1, 1) from one continuous action (O = 4, A = 1, action space
// [-1, 1], reward 1 per step, termination when |x| > 2.4 or |theta| > 12 degrees, 500-step
// truncation). The arithmetic is include/ppo_cartpole.h, shared with the device env
// (include/ppo_synth_env.h, PSYN_CARTPOLE), so host and device trajectories are bit-identical
// (compile with -ffp-contract=off). Reset noise as Pendulum's: Philox4x32-10 keyed
// (seed, 0x5EED5EED), counter (resets, i), i = 0..3 for x, xdot, theta, thetadot.
#pragma once

#include <cstdint>

#include "../../include/ppo_cartpole.h"
#include "gym.h"
#include "synthetic_cheetah.h"  // philox4x32_host

namespace gymcpp {

class CartPoleContinuous final : public Environment {
  float s_[CART_OBS_DIM] = {0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t rseed_ = 1, rcount_ = 0;
  int elapsed_ = CART_MAX_STEPS + 1;

 public:
  // seed > 0 re-keys the reset noise; otherwise the reset count continues
  ObsView reset(int seed) override {
    if (seed > 0) { rseed_ = (uint32_t)seed; rcount_ = 0; }
    float u[CART_OBS_DIM];
    for (int i = 0; i < CART_OBS_DIM; ++i) {
      uint32_t r[4];
      philox4x32_host(rcount_, (uint32_t)i, 0u, 0u, rseed_, 0x5EED5EEDu, r);
      u[i] = ((float)(r[0] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    }
    cart_reset(u, s_);
    rcount_ += 1;
    elapsed_ = 0;
    return ObsView{s_, CART_OBS_DIM};
  }
  std::tuple<ObsView, float, bool, bool> step(const float* a) override {
    float term = 0.0f;
    const float reward = cart_step(s_, a[0], &term);
    ++elapsed_;
    return {ObsView{s_, CART_OBS_DIM}, reward, term != 0.0f, elapsed_ >= CART_MAX_STEPS};
  }
  int get_observation_space() const override { return CART_OBS_DIM; }
  int get_action_space() const override { return CART_ACT_DIM; }
  float get_action_space_min() const override { return -1.0f; }
  float get_action_space_max() const override { return 1.0f; }
  const float* state() const { return s_; }
  void set_state(const float* s) {
    for (int i = 0; i < CART_OBS_DIM; ++i) s_[i] = s[i];
    elapsed_ = 0;
  }
};

}  // namespace gymcpp
