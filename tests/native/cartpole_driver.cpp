// Test driver for the host CartPoleContinuous-v1 (include/ppo_cartpole.h, ppo.cpp_amd/gymcpp/cartpole.h).
//   cartpole_driver step    in.f32 out.f32          in: (x, xdot, theta, thetadot, a)[n]
//                                                   out: (x', xdot', theta', thetadot', reward, term)[n]
//   cartpole_driver vec     E T seed clip act.f32 out.f32
//   cartpole_driver vecw    E T seed clip act.f32 out.f32 gamma
//   cartpole_driver balance E T seed out.f32        vec, with the driver's own balancing actions
//                                                   a = clip(3 theta + thetadot + 0.1 x + 0.2 xdot, -1, 1)
//                                                   of each env's observation (theta and thetadot alone
//                                                   balance the pole but let the cart drift to |x| = 2.4)
// vec: SeqVectorEnv over RecordEpisodeStatistics(CartPoleContinuous); vecw: over the PPO wrapper chain
// (make_env). out: obs0[E*4], then per step obs[E*4], reward[E], term[E], trunc[E], info_ret[E],
// info_len[E] (the layout of host_env_driver.cpp and pendulum_driver.cpp).
// Built as a shared object (-shared -fPIC) the same file gives scripts/cartpole_learning_ref.py its
// vector env: cartdrv_create / cartdrv_reset / cartdrv_step / cartdrv_destroy.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../ppo.cpp_amd/gymcpp/cartpole.h"
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

// act == nullptr: the balancing controller on the (unwrapped) observation
static int run_vec(bool wrapped, int E, int T, int seed, bool clip, float gamma, const std::vector<float>* act,
                   FILE* out) {
  std::vector<std::shared_ptr<gymcpp::EnvironmentWrapper>> envs;
  for (int e = 0; e < E; ++e) {
    auto base = std::make_shared<gymcpp::CartPoleContinuous>();
    if (wrapped) envs.push_back(gymcpp::make_env(base, gamma));
    else envs.push_back(std::make_shared<gymcpp::RecordEpisodeStatistics>(base));
  }
  gymcpp::SeqVectorEnv venv(envs, clip);
  const int O = venv.get_observation_space(), A = venv.get_action_space();
  if (act && (long)act->size() != (long)T * E * A) return 3;
  const float* o = venv.reset(seed);
  fwrite(o, sizeof(float), (size_t)E * O, out);
  std::vector<float> ir(E), il(E), ctl((size_t)E * A), cur(o, o + (size_t)E * O);
  for (int t = 0; t < T; ++t) {
    if (!act)
      for (int e = 0; e < E; ++e) {
        const float* c = cur.data() + (size_t)e * O;
        ctl[e] = std::min(1.0f, std::max(-1.0f, ((3.0f * c[2]) + c[3]) + ((0.1f * c[0]) + (0.2f * c[1]))));
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
    std::vector<float> o(n * 6);
    for (size_t i = 0; i < n; ++i) {
      float* r = o.data() + 6 * i;
      for (int k = 0; k < 4; ++k) r[k] = in[5 * i + k];
      r[4] = cart_step(r, in[5 * i + 4], &r[5]);
    }
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 4;
    fwrite(o.data(), sizeof(float), o.size(), out);
    fclose(out);
    return 0;
  }
  if (mode == "balance" && argc == 6) {
    const int E = std::atoi(argv[2]), T = std::atoi(argv[3]), seed = std::atoi(argv[4]);
    if (E <= 0 || T < 0) return 2;
    FILE* out = fopen(argv[5], "wb");
    if (!out) return 4;
    const int rc = run_vec(false, E, T, seed, true, 0.99f, nullptr, out);
    fclose(out);
    return rc;
  }
  if ((mode == "vec" && argc == 8) || (mode == "vecw" && argc == 9)) {
    const int E = std::atoi(argv[2]), T = std::atoi(argv[3]), seed = std::atoi(argv[4]);
    const bool clip = std::atoi(argv[5]) != 0;
    const float gamma = mode == "vecw" ? (float)std::atof(argv[8]) : 0.99f;
    if (E <= 0 || T < 0) return 2;
    const std::vector<float> act = read_f32(argv[6]);
    FILE* out = fopen(argv[7], "wb");
    if (!out) return 4;
    const int rc = run_vec(mode == "vecw", E, T, seed, clip, gamma, &act, out);
    fclose(out);
    return rc;
  }
  return 2;
}

// ---- the same vector env as a C interface (shared-object build) ----
struct cartdrv {
  std::unique_ptr<gymcpp::SeqVectorEnv> venv;
  int E;
};
extern "C" {
cartdrv* cartdrv_create(int E, int clip_actions) {
  if (E <= 0) return nullptr;
  std::vector<std::shared_ptr<gymcpp::EnvironmentWrapper>> envs;
  for (int e = 0; e < E; ++e)
    envs.push_back(std::make_shared<gymcpp::RecordEpisodeStatistics>(std::make_shared<gymcpp::CartPoleContinuous>()));
  auto* p = new cartdrv();
  p->venv = std::make_unique<gymcpp::SeqVectorEnv>(envs, clip_actions != 0);
  p->E = E;
  return p;
}
void cartdrv_destroy(cartdrv* p) { delete p; }
void cartdrv_reset(cartdrv* p, int seed, float* obs) {
  const float* o = p->venv->reset(seed);
  std::memcpy(obs, o, sizeof(float) * (size_t)p->E * 4);
}
// done = term | trunc; info_ret / info_len: the finished episode's return / length, else 0
void cartdrv_step(cartdrv* p, const float* act, float* obs, float* reward, float* term, float* done, float* info_ret,
                  float* info_len) {
  gymcpp::VecStep r = p->venv->step(act);
  std::memcpy(obs, r.obs, sizeof(float) * (size_t)p->E * 4);
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
