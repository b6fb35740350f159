// Test driver for the host Pendulum-v1 (include/ppo_pendulum.h, ppo.cpp_amd/gymcpp/pendulum.h).
//   pendulum_driver sincos in.f32 out.f32          in: x[n]              out: sin[n], cos[n]
//   pendulum_driver step   in.f32 out.f32          in: (theta, thetadot, a)[n]
//                                                  out: (obs[3], reward, theta', thetadot')[n]
//   pendulum_driver free   T seed act.f32 out.f32  one env, reset(seed), T steps of act[T]
//                                                  out: (theta, thetadot, reward)[T]
//   pendulum_driver vec    E T seed clip act.f32 out.f32
//   pendulum_driver vecw   E T seed clip act.f32 out.f32 gamma
// vec: SeqVectorEnv over RecordEpisodeStatistics(Pendulum); vecw: over the PPO wrapper chain
// (make_env). out: obs0[E*3], then per step obs[E*3], reward[E], term[E], trunc[E], info_ret[E],
// info_len[E] (the layout of host_env_driver.cpp).
// Built as a shared object (-shared -fPIC) the same file gives scripts/pendulum_learning_ref.py its
// vector env: pendrv_create / pendrv_reset / pendrv_step / pendrv_destroy.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../ppo.cpp_amd/gymcpp/gym.h"
#include "../../ppo.cpp_amd/gymcpp/pendulum.h"
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

static int run_vec(bool wrapped, int E, int T, int seed, bool clip, float gamma, const std::vector<float>& act,
                   FILE* out) {
  std::vector<std::shared_ptr<gymcpp::EnvironmentWrapper>> envs;
  for (int e = 0; e < E; ++e) {
    auto base = std::make_shared<gymcpp::Pendulum>();
    if (wrapped) envs.push_back(gymcpp::make_env(base, gamma));
    else envs.push_back(std::make_shared<gymcpp::RecordEpisodeStatistics>(base));
  }
  gymcpp::SeqVectorEnv venv(envs, clip);
  const int O = venv.get_observation_space(), A = venv.get_action_space();
  if ((long)act.size() != (long)T * E * A) return 3;
  const float* o = venv.reset(seed);
  fwrite(o, sizeof(float), (size_t)E * O, out);
  std::vector<float> ir(E), il(E);
  for (int t = 0; t < T; ++t) {
    gymcpp::VecStep r = venv.step(act.data() + (size_t)t * E * A);
    for (int e = 0; e < E; ++e) {
      const auto& inf = (*r.infos)[e];
      ir[e] = inf ? inf->r : 0.f;
      il[e] = inf ? (float)inf->l : 0.f;
    }
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
  if (mode == "sincos" && argc == 4) {
    const std::vector<float> x = read_f32(argv[2]);
    std::vector<float> s(x.size()), c(x.size());
    for (size_t i = 0; i < x.size(); ++i) pend_sincos(x[i], &s[i], &c[i]);
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 4;
    fwrite(s.data(), sizeof(float), s.size(), out);
    fwrite(c.data(), sizeof(float), c.size(), out);
    fclose(out);
    return 0;
  }
  if (mode == "step" && argc == 4) {
    const std::vector<float> in = read_f32(argv[2]);
    const size_t n = in.size() / 3;
    std::vector<float> o(n * 6);
    for (size_t i = 0; i < n; ++i) {
      float th = in[3 * i], thd = in[3 * i + 1];
      float* r = o.data() + 6 * i;
      r[3] = pend_step(&th, &thd, in[3 * i + 2], r);
      r[4] = th;
      r[5] = thd;
    }
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 4;
    fwrite(o.data(), sizeof(float), o.size(), out);
    fclose(out);
    return 0;
  }
  if (mode == "free" && argc == 6) {
    const int T = std::atoi(argv[2]), seed = std::atoi(argv[3]);
    const std::vector<float> act = read_f32(argv[4]);
    if ((int)act.size() != T) return 3;
    gymcpp::Pendulum env;
    env.reset(seed);
    std::vector<float> o((size_t)T * 3);
    for (int t = 0; t < T; ++t) {
      auto [ov, r, te, tr] = env.step(&act[t]);
      (void)ov; (void)te; (void)tr;
      o[3 * t] = env.theta();
      o[3 * t + 1] = env.theta_dot();
      o[3 * t + 2] = r;
    }
    FILE* out = fopen(argv[5], "wb");
    if (!out) return 4;
    fwrite(o.data(), sizeof(float), o.size(), out);
    fclose(out);
    return 0;
  }
  if ((mode == "vec" && argc == 8) || (mode == "vecw" && argc == 9)) {
    const int E = std::atoi(argv[2]), T = std::atoi(argv[3]), seed = std::atoi(argv[4]);
    const bool clip = std::atoi(argv[5]) != 0;
    const float gamma = mode == "vecw" ? (float)std::atof(argv[8]) : 0.99f;
    if (E <= 0 || T < 0) return 2;
    const std::vector<float> act = read_f32(argv[6]);
    FILE* out = fopen(argv[7], "wb");
    if (!out) return 4;
    const int rc = run_vec(mode == "vecw", E, T, seed, clip, gamma, act, out);
    fclose(out);
    return rc;
  }
  return 2;
}

// ---- the same vector env as a C interface (shared-object build) ----
struct pendrv {
  std::unique_ptr<gymcpp::SeqVectorEnv> venv;
  int E;
};
extern "C" {
pendrv* pendrv_create(int E, int clip_actions) {
  if (E <= 0) return nullptr;
  std::vector<std::shared_ptr<gymcpp::EnvironmentWrapper>> envs;
  for (int e = 0; e < E; ++e)
    envs.push_back(std::make_shared<gymcpp::RecordEpisodeStatistics>(std::make_shared<gymcpp::Pendulum>()));
  auto* p = new pendrv();
  p->venv = std::make_unique<gymcpp::SeqVectorEnv>(envs, clip_actions != 0);
  p->E = E;
  return p;
}
void pendrv_destroy(pendrv* p) { delete p; }
void pendrv_reset(pendrv* p, int seed, float* obs) {
  const float* o = p->venv->reset(seed);
  std::memcpy(obs, o, sizeof(float) * (size_t)p->E * 3);
}
// done = term | trunc; info_ret / info_len: the finished episode's return / length, else 0
void pendrv_step(pendrv* p, const float* act, float* obs, float* reward, float* done, float* info_ret,
                 float* info_len) {
  gymcpp::VecStep r = p->venv->step(act);
  std::memcpy(obs, r.obs, sizeof(float) * (size_t)p->E * 3);
  for (int e = 0; e < p->E; ++e) {
    reward[e] = r.rewards[e];
    done[e] = (r.terminations[e] != 0.f || r.truncations[e] != 0.f) ? 1.f : 0.f;
    const auto& inf = (*r.infos)[e];
    info_ret[e] = inf ? inf->r : 0.f;
    info_len[e] = inf ? (float)inf->l : 0.f;
  }
}
}
