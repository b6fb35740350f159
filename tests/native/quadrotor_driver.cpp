// Test driver for the host QuadrotorHover-v0 (include/ppo_quadrotor.h, ppo.cpp_amd/gymcpp/quadrotor.h):
// the textbook Newton-Euler quadrotor hovering at the origin (the project's own task).
//   quadrotor_driver step  in.f32 out.f32          in: (state[13], a[4])[n]
//                                                  out: (state'[13], reward, term, obs[18])[n]
//   quadrotor_driver reset seed n out.f32          state[13][n] of the resets 0 .. n-1 of one env keyed seed
//   quadrotor_driver draws u.f32 out.f32           quad_reset of the given uniforms (u[12])[n]: state[13][n]
//   quadrotor_driver vec   E T seed clip act.f32 out.f32
//   quadrotor_driver vecw  E T seed clip act.f32 out.f32 gamma
// vec: SeqVectorEnv over RecordEpisodeStatistics(QuadrotorHover); vecw: over the PPO wrapper chain
// (make_env). out: obs0[E*18], then per step obs[E*18], reward[E], term[E], trunc[E], info_ret[E],
// info_len[E] (the layout of host_env_driver.cpp, pendulum_driver.cpp, cartpole_driver.cpp and
// reacher_driver.cpp).
// Built as a shared object (-shared -fPIC) the same file gives scripts/quadrotor_learning_ref.py and
// the closed-loop tests their vector env: quaddrv_create / quaddrv_reset / quaddrv_step /
// quaddrv_destroy.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../ppo.cpp_amd/gymcpp/gym.h"
#include "../../ppo.cpp_amd/gymcpp/quadrotor.h"
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
    auto base = std::make_shared<gymcpp::QuadrotorHover>();
    if (wrapped) envs.push_back(gymcpp::make_env(base, gamma));
    else envs.push_back(std::make_shared<gymcpp::RecordEpisodeStatistics>(base));
  }
  gymcpp::SeqVectorEnv venv(envs, clip);
  const int O = venv.get_observation_space(), A = venv.get_action_space();
  if (O != QUAD_OBS_DIM || A != QUAD_ACT_DIM) return 5;
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
  if (mode == "step" && argc == 4) {
    const std::vector<float> in = read_f32(argv[2]);
    const int NI = QUAD_STATE_DIM + QUAD_ACT_DIM, NO = QUAD_STATE_DIM + 2 + QUAD_OBS_DIM;
    const size_t n = in.size() / NI;
    std::vector<float> o(n * NO);
    for (size_t i = 0; i < n; ++i) {
      float* r = o.data() + NO * i;
      for (int k = 0; k < QUAD_STATE_DIM; ++k) r[k] = in[NI * i + k];
      r[QUAD_STATE_DIM] = quad_step(r, &in[NI * i + QUAD_STATE_DIM], r + QUAD_STATE_DIM + 2, r + QUAD_STATE_DIM + 1);
    }
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 4;
    fwrite(o.data(), sizeof(float), o.size(), out);
    fclose(out);
    return 0;
  }
  if (mode == "draws" && argc == 4) {
    const std::vector<float> in = read_f32(argv[2]);
    const size_t n = in.size() / QUAD_RESET_DRAWS;
    std::vector<float> o(n * QUAD_STATE_DIM);
    for (size_t i = 0; i < n; ++i) quad_reset(&in[QUAD_RESET_DRAWS * i], o.data() + QUAD_STATE_DIM * i);
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 4;
    fwrite(o.data(), sizeof(float), o.size(), out);
    fclose(out);
    return 0;
  }
  if (mode == "reset" && argc == 5) {
    const int seed = std::atoi(argv[2]), n = std::atoi(argv[3]);
    if (seed <= 0 || n <= 0) return 2;
    gymcpp::QuadrotorHover env;
    FILE* out = fopen(argv[4], "wb");
    if (!out) return 4;
    for (int i = 0; i < n; ++i) {
      env.reset(i == 0 ? seed : 0);
      fwrite(env.state(), sizeof(float), QUAD_STATE_DIM, out);
    }
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
struct quaddrv {
  std::unique_ptr<gymcpp::SeqVectorEnv> venv;
  int E;
};
extern "C" {
quaddrv* quaddrv_create(int E, int clip_actions) {
  if (E <= 0) return nullptr;
  std::vector<std::shared_ptr<gymcpp::EnvironmentWrapper>> envs;
  for (int e = 0; e < E; ++e)
    envs.push_back(std::make_shared<gymcpp::RecordEpisodeStatistics>(std::make_shared<gymcpp::QuadrotorHover>()));
  auto* p = new quaddrv();
  p->venv = std::make_unique<gymcpp::SeqVectorEnv>(envs, clip_actions != 0);
  p->E = E;
  return p;
}
void quaddrv_destroy(quaddrv* p) { delete p; }
void quaddrv_reset(quaddrv* p, int seed, float* obs) {
  const float* o = p->venv->reset(seed);
  std::memcpy(obs, o, sizeof(float) * (size_t)p->E * QUAD_OBS_DIM);
}
// done = term | trunc; info_ret / info_len: the finished episode's return / length, else 0
void quaddrv_step(quaddrv* p, const float* act, float* obs, float* reward, float* term, float* done, float* info_ret,
                  float* info_len) {
  gymcpp::VecStep r = p->venv->step(act);
  std::memcpy(obs, r.obs, sizeof(float) * (size_t)p->E * QUAD_OBS_DIM);
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
