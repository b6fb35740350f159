// gymcpp/pendulum.h — Gymnasium's Pendulum-v1 (O = 3, A = 1, torque in [-2, 2], 200-step truncation,
// never terminates) behind the Environment interface. The arithmetic is include/ppo_pendulum.h,
// shared with the device env (include/ppo_synth_env.h, PSYN_PENDULUM), so host and device
// trajectories are bit-identical (compile with -ffp-contract=off). Reset noise as SyntheticCheetah's:
// Philox4x32-10 keyed (seed, 0x5EED5EED), counter (resets, i), i = 0 for the angle, 1 for the speed.
#pragma once

#include <cstdint>

#include "../../include/ppo_pendulum.h"
#include "gym.h"
#include "synthetic_cheetah.h"  // philox4x32_host

namespace gymcpp {

class Pendulum final : public Environment {
  float th_ = 0.0f, thd_ = 0.0f;
  float obs_[PEND_OBS_DIM] = {1.0f, 0.0f, 0.0f};
  uint32_t rseed_ = 1, rcount_ = 0;
  int elapsed_ = PEND_MAX_STEPS + 1;

 public:
  // seed > 0 re-keys the reset noise; otherwise the reset count continues
  ObsView reset(int seed) override {
    if (seed > 0) { rseed_ = (uint32_t)seed; rcount_ = 0; }
    float u[2];
    for (int i = 0; i < 2; ++i) {
      uint32_t r[4];
      philox4x32_host(rcount_, (uint32_t)i, 0u, 0u, rseed_, 0x5EED5EEDu, r);
      u[i] = ((float)(r[0] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    }
    pend_reset(u[0], u[1], &th_, &thd_);
    pend_obs(th_, thd_, obs_);
    rcount_ += 1;
    elapsed_ = 0;
    return ObsView{obs_, PEND_OBS_DIM};
  }
  std::tuple<ObsView, float, bool, bool> step(const float* a) override {
    const float reward = pend_step(&th_, &thd_, a[0], obs_);
    ++elapsed_;
    return {ObsView{obs_, PEND_OBS_DIM}, reward, false, elapsed_ >= PEND_MAX_STEPS};
  }
  int get_observation_space() const override { return PEND_OBS_DIM; }
  int get_action_space() const override { return PEND_ACT_DIM; }
  float get_action_space_min() const override { return -PEND_MAX_TORQUE; }
  float get_action_space_max() const override { return PEND_MAX_TORQUE; }
  float theta() const { return th_; }
  float theta_dot() const { return thd_; }
  void set_state(float th, float thd) { th_ = th; thd_ = thd; elapsed_ = 0; }
};

}  // namespace gymcpp
