// Test driver for the host AcrobotContinuous-v1 (include/ppo_acrobot.h, ppo.cpp_amd/gymcpp/acrobot.h).
//   acrobot_driver step   in.f32 out.f32          in: (theta1, theta2, theta1dot, theta2dot, a)[n]
//                                                 out: (state'[4], obs'[6], reward, term)[n]
//   acrobot_driver reduce in.f32 out.f32          in: x[n]; out: (acro_reduce(x), pend_wrap of it, and
//                                                 pend_sincos's sin and cos of acro_reduce(x))[n]
//   acrobot_driver vec    E T seed clip act.f32 out.f32
//   acrobot_driver vecw   E T seed clip act.f32 out.f32 gamma
//   acrobot_driver pump   E T seed noise_seed out.f32 act.f32
//                                                 vec (clip on), with the driver's own energy-pumping
//                                                 actions, which it records in act.f32 [T, E]:
//                                                 a = sign(theta2dot) + (u - 0.5), u uniform in [0, 1)
//                                                 from mt19937(noise_seed), one draw per env and step;
//                                                 every ninth env (e % 9 == 8) gets the noise alone and
//                                                 never swings up, so its episodes end by truncation
// vec: SeqVectorEnv over RecordEpisodeStatistics(AcrobotContinuous); vecw: over the PPO wrapper chain
// (make_env). out: obs0[E*6], then per step obs[E*6], reward[E], term[E], trunc[E], info_ret[E],
// info_len[E] (the layout of host_env_driver.cpp and pendulum_driver.cpp).
// Built as a shared object (-shared -fPIC) the same file gives scripts/acrobot_learning_ref.py its
// vector env: acrodrv_create / acrodrv_reset / acrodrv_step / acrodrv_destroy.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../ppo.cpp_amd/gymcpp/acrobot.h"
#include "../../ppo.cpp_amd/gymcpp/gym.h"
#include "../../ppo.cpp_amd/gymcpp/wrappers.h"

static std::vector<float> read_f32(const char* path) {
  std::vector<float> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f) / (long)sizeof(float);
  fseek(f, 0, SEEK_SET);
  v.resize((size_t)n);
  if (n > 0 && fread(v.data(), sizeof(float), (size_t)n, f) != (size_t)n) v.clear();
  fclose(f);
  return v;
}

static bool write_f32(const char* path, const std::vector<float>& v) {
  FILE* out = fopen(path, "wb");
  if (!out) return false;
  fwrite(v.data(), sizeof(float), v.size(), out);
  fclose(out);
  return true;
}

// act == nullptr: the energy-pumping rule on the (unwrapped) observation, recorded in *rec
static int run_vec(bool wrapped, int E, int T, int seed, bool clip, float gamma, const std::vector<float>* act,
                   unsigned noise_seed, std::vector<float>* rec, FILE* out) {
  std::vector<std::shared_ptr<gymcpp::EnvironmentWrapper>> envs;
  for (int e = 0; e < E; ++e) {
    auto base = std::make_shared<gymcpp::AcrobotContinuous>();
    if (wrapped) envs.push_back(gymcpp::make_env(base, gamma));
    else envs.push_back(std::make_shared<gymcpp::RecordEpisodeStatistics>(base));
  }
  gymcpp::SeqVectorEnv venv(envs, clip);
  const int O = venv.get_observation_space(), A = venv.get_action_space();
  if (act && (long)act->size() != (long)T * E * A) return 3;
  const float* o = venv.reset(seed);
  fwrite(o, sizeof(float), (size_t)E * O, out);
  std::vector<float> ir(E), il(E), ctl((size_t)E * A), cur(o, o + (size_t)E * O);
  std::mt19937 gen(noise_seed);
  for (int t = 0; t < T; ++t) {
    if (!act) {
      for (int e = 0; e < E; ++e) {
        const float w2 = cur[(size_t)e * O + 5];
        const float noise = ((float)(gen() >> 8) * 5.9604644775390625e-8f) - 0.5f;
        const float push = (e % 9 == 8) ? 0.0f : (w2 > 0.0f ? 1.0f : (w2 < 0.0f ? -1.0f : 0.0f));
        ctl[e] = push + noise;
      }
      rec->insert(rec->end(), ctl.begin(), ctl.end());
    }
    gymcpp::VecStep r = venv.step(act ? act->data() + (size_t)t * E * A : ctl.data());
    for (int e = 0; e < E; ++e) {
      const auto& inf = (*r.infos)[e];
      ir[e] = inf ? inf->r : 0.f;
      il[e] = inf ? (float)inf->l : 0.f;
    }
    cur.assign(r.obs, r.obs + (size_t)E * O);
    fwrite(r.obs, sizeof(float), (size_t)E * O, out);
    fwrite(r.rewards, sizeof(float), E, out);
    fwrite(r.terminations, sizeof(float), E, out);
    fwrite(r.truncations, sizeof(float), E, out);
    fwrite(ir.data(), sizeof(float), E, out);
    fwrite(il.data(), sizeof(float), E, out);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::string mode = argv[1];
  if (mode == "step" && argc == 4) {
    const std::vector<float> in = read_f32(argv[2]);
    const size_t n = in.size() / 5;
    std::vector<float> o(n * 12);
    for (size_t i = 0; i < n; ++i) {
      float* r = o.data() + 12 * i;
      for (int k = 0; k < 4; ++k) r[k] = in[5 * i + k];
      r[10] = acro_step(r, in[5 * i + 4], r + 4, &r[11]);
    }
    return write_f32(argv[3], o) ? 0 : 4;
  }
  if (mode == "reduce" && argc == 4) {
    const std::vector<float> in = read_f32(argv[2]);
    std::vector<float> o(in.size() * 4);
    for (size_t i = 0; i < in.size(); ++i) {
      float* r = o.data() + 4 * i;
      r[0] = acro_reduce(in[i]);
      r[1] = pend_wrap(r[0]);
      pend_sincos(r[0], &r[2], &r[3]);
    }
    return write_f32(argv[3], o) ? 0 : 4;
  }
  if (mode == "pump" && argc == 8) {
    const int E = std::atoi(argv[2]), T = std::atoi(argv[3]), seed = std::atoi(argv[4]);
    if (E <= 0 || T < 0) return 2;
    FILE* out = fopen(argv[6], "wb");
    if (!out) return 4;
    std::vector<float> rec;
    const int rc = run_vec(false, E, T, seed, true, 0.99f, nullptr, (unsigned)std::atoi(argv[5]), &rec, out);
    fclose(out);
    if (rc) return rc;
    return write_f32(argv[7], rec) ? 0 : 4;
  }
  if ((mode == "vec" && argc == 8) || (mode == "vecw" && argc == 9)) {
    const int E = std::atoi(argv[2]), T = std::atoi(argv[3]), seed = std::atoi(argv[4]);
    const bool clip = std::atoi(argv[5]) != 0;
    const float gamma = mode == "vecw" ? (float)std::atof(argv[8]) : 0.99f;
    if (E <= 0 || T < 0) return 2;
    const std::vector<float> act = read_f32(argv[6]);
    FILE* out = fopen(argv[7], "wb");
    if (!out) return 4;
    const int rc = run_vec(mode == "vecw", E, T, seed, clip, gamma, &act, 0u, nullptr, out);
    fclose(out);
    return rc;
  }
  return 2;
}

// ---- the same vector env as a C interface (shared-object build) ----
struct acrodrv {
  std::unique_ptr<gymcpp::SeqVectorEnv> venv;
  int E;
};
extern "C" {
acrodrv* acrodrv_create(int E, int clip_actions) {
  if (E <= 0) return nullptr;
  std::vector<std::shared_ptr<gymcpp::EnvironmentWrapper>> envs;
  for (int e = 0; e < E; ++e)
    envs.push_back(std::make_shared<gymcpp::RecordEpisodeStatistics>(std::make_shared<gymcpp::AcrobotContinuous>()));
  auto* p = new acrodrv();
  p->venv = std::make_unique<gymcpp::SeqVectorEnv>(envs, clip_actions != 0);
  p->E = E;
  return p;
}
void acrodrv_destroy(acrodrv* p) { delete p; }
void acrodrv_reset(acrodrv* p, int seed, float* obs) {
  const float* o = p->venv->reset(seed);
  std::memcpy(obs, o, sizeof(float) * (size_t)p->E * ACRO_OBS_DIM);
}
// done = term | trunc; info_ret / info_len: the finished episode's return / length, else 0
void acrodrv_step(acrodrv* p, const float* act, float* obs, float* reward, float* term, float* done, float* info_ret,
                  float* info_len) {
  gymcpp::VecStep r = p->venv->step(act);
  std::memcpy(obs, r.obs, sizeof(float) * (size_t)p->E * ACRO_OBS_DIM);
  for (int e = 0; e < p->E; ++e) {
    reward[e] = r.rewards[e];
    term[e] = r.terminations[e];
    done[e] = (r.terminations[e] != 0.f || r.truncations[e] != 0.f) ? 1.f : 0.f;
    const auto& inf = (*r.infos)[e];
    info_ret[e] = inf ? inf->r : 0.f;
    info_len[e] = inf ? (float)inf->l : 0.f;
  }
}
}
