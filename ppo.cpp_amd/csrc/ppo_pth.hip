// ppo_pth.hip — C-ABI of include/ppo_pth.h: the reference agents' module structure as pth::Spec
// over the flat layouts, and the archive reader/writer of pth_io.hpp. Host code only.
#include <algorithm>
#include <exception>
#include <string>
#include <vector>

#include "../../include/ppo_pth.h"
#include "ppo_kernels.hpp"  // ppo_fail
#include "pth_io.hpp"

namespace {

using Shape = std::vector<int64_t>;

void seq(pth::Spec& s, const std::string& name, int n) {
  s.modules.push_back(name);
  for (int i = 0; i < n; ++i) s.modules.push_back(name + "." + std::to_string(i));
}
void linear(pth::Spec& s, const std::string& name, long w, long b, int out, int in) {
  s.tensors.push_back({name + ".weight", Shape{out, in}, w, true});
  s.tensors.push_back({name + ".bias", Shape{out}, b, true});
}
void norm(pth::Spec& s, const std::string& name, long g, long b, int n) {
  s.tensors.push_back({name + ".weight", Shape{n}, g, true});
  s.tensors.push_back({name + ".bias", Shape{n}, b, true});
}

// ppo_continuous_action.cpp:120-157 / ac_ppo_continuous_action.cpp:150-249
pth::Spec agent_spec(const ppo_layout& L) {
  pth::Spec s;
  s.P = L.P;
  const int O = L.O, A = L.A, H = L.H;
  if (L.kind == PPO_NET_TANH_NORMAL) {
    seq(s, "critic", 5);      // Linear Tanh Linear Tanh Linear
    seq(s, "actor_mean", 5);
    s.tensors.push_back({"actor_logstd", Shape{1, A}, L.logstd, true});
    linear(s, "critic.0", L.critic.W1, L.critic.b1, H, O);
    linear(s, "critic.2", L.critic.W2, L.critic.b2, H, H);
    linear(s, "critic.4", L.cW3, L.cb3, 1, H);
    linear(s, "actor_mean.0", L.actor.W1, L.actor.b1, H, O);
    linear(s, "actor_mean.2", L.actor.W2, L.actor.b2, H, H);
    linear(s, "actor_mean.4", L.aW3, L.ab3, A, H);
  } else {
    seq(s, "critic", 7);      // Linear LayerNorm ReLU Linear LayerNorm ReLU Linear
    seq(s, "actor_mean", 6);  // Linear LayerNorm ReLU Linear LayerNorm ReLU
    seq(s, "dist_alpha", 1);
    seq(s, "dist_beta", 1);
    s.tensors.push_back({"action_space_high", Shape{}, L.hi, false});
    s.tensors.push_back({"action_space_low", Shape{}, L.lo, false});
    s.tensors.push_back({"mean_", Shape{1, O}, L.omean, false});
    s.tensors.push_back({"std_", Shape{1, O}, L.ostd, false});
    linear(s, "critic.0", L.critic.W1, L.critic.b1, H, O);
    norm(s, "critic.1", L.critic.g1, L.critic.be1, H);
    linear(s, "critic.3", L.critic.W2, L.critic.b2, H, H);
    norm(s, "critic.4", L.critic.g2, L.critic.be2, H);
    linear(s, "critic.6", L.cW3, L.cb3, 1, H);
    linear(s, "actor_mean.0", L.actor.W1, L.actor.b1, H, O);
    norm(s, "actor_mean.1", L.actor.g1, L.actor.be1, H);
    linear(s, "actor_mean.3", L.actor.W2, L.actor.b2, H, H);
    norm(s, "actor_mean.4", L.actor.g2, L.actor.be2, H);
    linear(s, "dist_alpha.0", L.aW3, L.ab3, A, H);
    linear(s, "dist_beta.0", L.bW3, L.bb3, A, H);
  }
  return s;
}

// carla_model.h:65-192 (roach encoder, no layer norm)
pth::Spec carla_spec(const ppo_carla_layout& L) {
  pth::Spec s;
  s.P = L.P;
  seq(s, "cnn", 2 * PPO_CARLA_NCONV);  // Conv ReLU x 6
  seq(s, "linear", 4);
  seq(s, "state_linear", 4);
  seq(s, "value_head", 5);
  seq(s, "policy_head", 4);
  seq(s, "dist_mu", 1);
  seq(s, "dist_sigma", 1);
  s.tensors.push_back({"action_space_high", Shape{}, L.hi, false});
  s.tensors.push_back({"action_space_low", Shape{}, L.lo, false});
  for (int i = 0; i < PPO_CARLA_NCONV; ++i) {
    const std::string n = "cnn." + std::to_string(2 * i);
    s.tensors.push_back({n + ".weight", Shape{L.conv_oc[i], L.conv_ic[i], L.conv_k[i], L.conv_k[i]}, L.conv_w[i], true});
    s.tensors.push_back({n + ".bias", Shape{L.conv_oc[i]}, L.conv_b[i], true});
  }
  linear(s, "linear.0", L.lin_w[0], L.lin_b[0], 512, 1024 + 256);
  linear(s, "linear.2", L.lin_w[1], L.lin_b[1], 256, 512);
  linear(s, "state_linear.0", L.st_w[0], L.st_b[0], 256, L.NM);
  linear(s, "state_linear.2", L.st_w[1], L.st_b[1], 256, 256);
  linear(s, "value_head.0", L.v_w[0], L.v_b[0], 256, 256 + L.NV);
  linear(s, "value_head.2", L.v_w[1], L.v_b[1], 256, 256);
  linear(s, "value_head.4", L.v_w[2], L.v_b[2], 1, 256);
  linear(s, "policy_head.0", L.pi_w[0], L.pi_b[0], 256, 256);
  linear(s, "policy_head.2", L.pi_w[1], L.pi_b[1], 256, 256);
  linear(s, "dist_mu.0", L.mu_w, L.mu_b, L.A, 256);
  linear(s, "dist_sigma.0", L.sg_w, L.sg_b, L.A, 256);
  return s;
}

// carla_model.h:44-192 for any ppo_carla_arch: a LayerNorm child after each normalised Conv2d / Linear
// shifts the Sequential indices (Conv LN ReLU: 3i, 3i + 1; Linear LN ReLU: 0, 1, 3, 4, 6). Tensors
// are pushed in the layout's named_parameters() order.
pth::Spec carla_spec2(const ppo_carla_layout2& L) {
  pth::Spec s;
  s.P = L.P;
  const int eln = L.arch.encoder_ln, mln = L.arch.mlp_ln, pln = L.arch.policy_ln;
  seq(s, "cnn", (eln ? 3 : 2) * PPO_CARLA_NCONV);
  seq(s, "linear", mln ? 6 : 4);
  seq(s, "state_linear", mln ? 6 : 4);
  seq(s, "value_head", mln ? 7 : 5);
  seq(s, "policy_head", pln ? 6 : 4);
  seq(s, "dist_mu", 1);
  seq(s, "dist_sigma", 1);
  s.tensors.push_back({"action_space_high", Shape{}, L.hi, false});
  s.tensors.push_back({"action_space_low", Shape{}, L.lo, false});
  for (int i = 0; i < PPO_CARLA_NCONV; ++i) {
    const int step = eln ? 3 : 2;
    const std::string n = "cnn." + std::to_string(step * i);
    s.tensors.push_back({n + ".weight", Shape{L.conv_oc[i], L.conv_ic[i], L.conv_k[i], L.conv_k[i]}, L.conv_w[i], true});
    s.tensors.push_back({n + ".bias", Shape{L.conv_oc[i]}, L.conv_b[i], true});
    if (eln) {
      const std::string m = "cnn." + std::to_string(step * i + 1);
      const Shape shp{L.conv_oc[i], L.conv_oh[i], L.conv_ow[i]};
      s.tensors.push_back({m + ".weight", shp, L.conv_g[i], true});
      s.tensors.push_back({m + ".bias", shp, L.conv_be[i], true});
    }
  }
  // a Sequential of Linear [LayerNorm] ReLU pairs: layer k at index k * (ln ? 3 : 2)
  auto mlp = [&](const std::string& name, int ln, int k, long w, long b, long g, long be, int out, int in) {
    const int at = k * (ln ? 3 : 2);
    linear(s, name + "." + std::to_string(at), w, b, out, in);
    if (ln && g >= 0) norm(s, name + "." + std::to_string(at + 1), g, be, out);
  };
  mlp("linear", mln, 0, L.lin_w[0], L.lin_b[0], L.lin_g[0], L.lin_be[0], 512, 1024 + 256);
  mlp("linear", mln, 1, L.lin_w[1], L.lin_b[1], L.lin_g[1], L.lin_be[1], 256, 512);
  mlp("state_linear", mln, 0, L.st_w[0], L.st_b[0], L.st_g[0], L.st_be[0], 256, L.NM);
  mlp("state_linear", mln, 1, L.st_w[1], L.st_b[1], L.st_g[1], L.st_be[1], 256, 256);
  mlp("value_head", mln, 0, L.v_w[0], L.v_b[0], L.v_g[0], L.v_be[0], 256, 256 + L.NV);
  mlp("value_head", mln, 1, L.v_w[1], L.v_b[1], L.v_g[1], L.v_be[1], 256, 256);
  mlp("value_head", mln, 2, L.v_w[2], L.v_b[2], -1, -1, 1, 256);
  mlp("policy_head", pln, 0, L.pi_w[0], L.pi_b[0], L.pi_g[0], L.pi_be[0], 256, 256);
  mlp("policy_head", pln, 1, L.pi_w[1], L.pi_b[1], L.pi_g[1], L.pi_be[1], 256, 256);
  linear(s, "dist_mu.0", L.mu_w, L.mu_b, L.A, 256);
  linear(s, "dist_sigma.0", L.sg_w, L.sg_b, L.A, 256);
  return s;
}

// the spec must tile the layout exactly (guards a layout / spec drift)
bool covers(const pth::Spec& s) {
  long total = 0;
  for (const auto& t : s.tensors) {
    long n = 1;
    for (int64_t d : t.shape) n *= (long)d;
    if (t.off < 0 || t.off + n > s.P) return false;
    total += n;
  }
  return total == s.P;
}

template <typename F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const std::exception& e) {
    return ppo_fail(e.what(), -1);
  }
}

}  // namespace

extern "C" int ppo_layout_fill(ppo_layout* L, int kind, int O, int A, int H) {
  if (!L || ppo_layout_init(L, kind, O, A, H) != 0) return ppo_fail("ppo_layout_fill: bad arguments", -1);
  return 0;
}

extern "C" int ppo_carla_layout_fill(ppo_carla_layout* L, int C, int IH, int IW, int NM, int NV, int A) {
  if (!L || ppo_carla_layout_init(L, C, IH, IW, NM, NV, A) != 0)
    return ppo_fail("ppo_carla_layout_fill: bad arguments (n_flatten must be 256 * 2 * 2)", -1);
  return 0;
}

extern "C" int ppo_carla_layout2_fill(ppo_carla_layout2* L, int C, int IH, int IW, int NM, int NV, int A,
                                      const ppo_carla_arch* arch) {
  return ppo_carla_layout2_fill_pos(L, C, IH, IW, NM, NV, A, arch, 0);
}

extern "C" int ppo_carla_layout2_fill_pos(ppo_carla_layout2* L, int C, int IH, int IW, int NM, int NV, int A,
                                          const ppo_carla_arch* arch, int pos_enc) {
  if (!L) return ppo_fail("ppo_carla_layout2_fill: null argument", -1);
  if (pos_enc != 0 && pos_enc != 1)
    return ppo_fail("ppo_carla_layout2_fill_pos: pos_enc must be 0 or 1 (use_positional_encoding)", -1);
  if (arch && (arch->encoder_ln < 0 || arch->encoder_ln > 1))
    return ppo_fail("ppo_carla_layout2_fill: encoder_ln must be 0 (roach) or 1 (roach_ln); roach_ln2 is not built", -1);
  const int rc = ppo_carla_layout2_init_pos(L, C, IH, IW, NM, NV, A, arch, pos_enc);
  if (rc == -2)
    return ppo_fail("ppo_carla_layout2_fill: the roach_ln encoder needs a 192 x 192 bev: the reference hard-codes its "
                    "LayerNorm shapes (carla_model.h:45-62)", -1);
  if (rc != 0) return ppo_fail("ppo_carla_layout2_fill: bad arguments (n_flatten must be 256 * 2 * 2)", -1);
  return 0;
}

extern "C" int ppo_carla_tensor_name(const ppo_carla_layout2* L, int t, char* buf, int len) {
  if (!L || !buf || len <= 0) return ppo_fail("ppo_carla_tensor_name: null argument", -1);
  if (t < 0 || t >= L->ntensors) return ppo_fail("ppo_carla_tensor_name: tensor index out of range", -1);
  return guarded([&] {
    const pth::Spec s = carla_spec2(*L);
    if ((int)s.tensors.size() != L->ntensors || s.tensors[t].off != L->t_off[t])
      return ppo_fail("ppo_carla_tensor_name: layout does not match the agent structure", -1);
    const std::string& nm = s.tensors[t].name;
    const size_t k = std::min(nm.size(), (size_t)len - 1);
    std::copy(nm.begin(), nm.begin() + k, buf);
    buf[k] = 0;
    return 0;
  });
}

extern "C" int ppo_pth_save_agent(const ppo_layout* L, const float* params, const char* path) {
  if (!L || !params || !path) return ppo_fail("ppo_pth_save_agent: null argument", -1);
  return guarded([&] {
    const pth::Spec s = agent_spec(*L);
    if (!covers(s)) return ppo_fail("ppo_pth_save_agent: layout does not match the agent structure", -1);
    pth::save_module(path, s, params);
    return 0;
  });
}

extern "C" int ppo_pth_load_agent(const ppo_layout* L, const char* path, float* params, long n) {
  if (!L || !params || !path) return ppo_fail("ppo_pth_load_agent: null argument", -1);
  if (n != L->P) return ppo_fail("ppo_pth_load_agent: n != layout P", -1);
  return guarded([&] {
    const pth::Spec s = agent_spec(*L);
    if (!covers(s)) return ppo_fail("ppo_pth_load_agent: layout does not match the agent structure", -1);
    const std::vector<float> flat = pth::load_module(path, s);
    std::copy(flat.begin(), flat.end(), params);
    return 0;
  });
}

extern "C" int ppo_pth_save_adam(const ppo_layout* L, const float* m, const float* v, long step, double lr,
                                 double eps, const char* path) {
  if (!L || !m || !v || !path) return ppo_fail("ppo_pth_save_adam: null argument", -1);
  if (step < 0) return ppo_fail("ppo_pth_save_adam: negative step", -1);
  return guarded([&] {
    const pth::Spec s = agent_spec(*L);
    pth::AdamOptions o;
    o.lr = lr;
    o.eps = eps;
    pth::save_adam(path, s, m, v, step, o);
    return 0;
  });
}

extern "C" int ppo_pth_load_adam(const ppo_layout* L, const char* path, float* m, float* v, long n, long* step,
                                 double* lr_out, double* eps_out) {
  if (!L || !m || !v || !path || !step) return ppo_fail("ppo_pth_load_adam: null argument", -1);
  if (n != L->P) return ppo_fail("ppo_pth_load_adam: n != layout P", -1);
  return guarded([&] {
    const pth::Spec s = agent_spec(*L);
    pth::AdamOptions o;
    *step = pth::load_adam(path, s, m, v, &o);
    if (lr_out) *lr_out = o.lr;
    if (eps_out) *eps_out = o.eps;
    return 0;
  });
}

extern "C" int ppo_carla_pth_save(const ppo_carla_layout* L, const float* params, const char* path) {
  if (!L || !params || !path) return ppo_fail("ppo_carla_pth_save: null argument", -1);
  return guarded([&] {
    const pth::Spec s = carla_spec(*L);
    if (!covers(s)) return ppo_fail("ppo_carla_pth_save: layout does not match the agent structure", -1);
    pth::save_module(path, s, params);
    return 0;
  });
}

extern "C" int ppo_carla_pth_load(const ppo_carla_layout* L, const char* path, float* params, long n) {
  if (!L || !params || !path) return ppo_fail("ppo_carla_pth_load: null argument", -1);
  if (n != L->P) return ppo_fail("ppo_carla_pth_load: n != layout P", -1);
  return guarded([&] {
    const pth::Spec s = carla_spec(*L);
    if (!covers(s)) return ppo_fail("ppo_carla_pth_load: layout does not match the agent structure", -1);
    const std::vector<float> flat = pth::load_module(path, s);
    std::copy(flat.begin(), flat.end(), params);
    return 0;
  });
}

extern "C" int ppo_carla_pth_save2(const ppo_carla_layout2* L, const float* params, const char* path) {
  if (!L || !params || !path) return ppo_fail("ppo_carla_pth_save2: null argument", -1);
  return guarded([&] {
    const pth::Spec s = carla_spec2(*L);
    if (!covers(s)) return ppo_fail("ppo_carla_pth_save2: layout does not match the agent structure", -1);
    pth::save_module(path, s, params);
    return 0;
  });
}

// torch::load into a module of another arch fails on the first parameter the archive lacks (a
// LayerNorm child where the layout expects none holds a ReLU, and the other way round), by name
extern "C" int ppo_carla_pth_load2(const ppo_carla_layout2* L, const char* path, float* params, long n) {
  if (!L || !params || !path) return ppo_fail("ppo_carla_pth_load2: null argument", -1);
  if (n != L->P) return ppo_fail("ppo_carla_pth_load2: n != layout P", -1);
  return guarded([&] {
    const pth::Spec s = carla_spec2(*L);
    if (!covers(s)) return ppo_fail("ppo_carla_pth_load2: layout does not match the agent structure", -1);
    const std::vector<float> flat = pth::load_module(path, s);
    std::copy(flat.begin(), flat.end(), params);
    return 0;
  });
}

// torch::save / torch::load of the CaRL trainer's Adam (ac_ppo_carla.cpp:62-73, :246-251)
extern "C" int ppo_carla_pth_save_adam2(const ppo_carla_layout2* L, const float* m, const float* v, long step,
                                        double lr, double eps, const char* path) {
  if (!L || !m || !v || !path) return ppo_fail("ppo_carla_pth_save_adam2: null argument", -1);
  if (step < 0) return ppo_fail("ppo_carla_pth_save_adam2: negative step", -1);
  return guarded([&] {
    const pth::Spec s = carla_spec2(*L);
    if (!covers(s)) return ppo_fail("ppo_carla_pth_save_adam2: layout does not match the agent structure", -1);
    pth::AdamOptions o;
    o.lr = lr;
    o.eps = eps;
    pth::save_adam(path, s, m, v, step, o);
    return 0;
  });
}

extern "C" int ppo_carla_pth_load_adam2(const ppo_carla_layout2* L, const char* path, float* m, float* v, long n,
                                        long* step, double* lr_out, double* eps_out) {
  if (!L || !m || !v || !path || !step) return ppo_fail("ppo_carla_pth_load_adam2: null argument", -1);
  if (n != L->P) return ppo_fail("ppo_carla_pth_load_adam2: n != layout P", -1);
  return guarded([&] {
    const pth::Spec s = carla_spec2(*L);
    if (!covers(s)) return ppo_fail("ppo_carla_pth_load_adam2: layout does not match the agent structure", -1);
    pth::AdamOptions o;
    *step = pth::load_adam(path, s, m, v, &o);
    if (lr_out) *lr_out = o.lr;
    if (eps_out) *eps_out = o.eps;
    return 0;
  });
}

// the same with the optimizer's betas and weight decay (ac_ppo_carla.cpp:246: Adam(lr).eps().weight_decay().betas())
extern "C" int ppo_carla_pth_save_adam3(const ppo_carla_layout2* L, const float* m, const float* v, long step,
                                        double lr, double eps, double beta1, double beta2, double weight_decay,
                                        const char* path) {
  if (!L || !m || !v || !path) return ppo_fail("ppo_carla_pth_save_adam3: null argument", -1);
  if (step < 0) return ppo_fail("ppo_carla_pth_save_adam3: negative step", -1);
  return guarded([&] {
    const pth::Spec s = carla_spec2(*L);
    if (!covers(s)) return ppo_fail("ppo_carla_pth_save_adam3: layout does not match the agent structure", -1);
    pth::AdamOptions o;
    o.lr = lr;
    o.eps = eps;
    o.beta1 = beta1;
    o.beta2 = beta2;
    o.weight_decay = weight_decay;
    pth::save_adam(path, s, m, v, step, o);
    return 0;
  });
}

extern "C" int ppo_carla_pth_load_adam3(const ppo_carla_layout2* L, const char* path, float* m, float* v, long n,
                                        long* step, double* lr_out, double* eps_out, double* beta1_out,
                                        double* beta2_out, double* weight_decay_out) {
  if (!L || !m || !v || !path || !step) return ppo_fail("ppo_carla_pth_load_adam3: null argument", -1);
  if (n != L->P) return ppo_fail("ppo_carla_pth_load_adam3: n != layout P", -1);
  return guarded([&] {
    const pth::Spec s = carla_spec2(*L);
    if (!covers(s)) return ppo_fail("ppo_carla_pth_load_adam3: layout does not match the agent structure", -1);
    pth::AdamOptions o;
    *step = pth::load_adam(path, s, m, v, &o);
    if (lr_out) *lr_out = o.lr;
    if (eps_out) *eps_out = o.eps;
    if (beta1_out) *beta1_out = o.beta1;
    if (beta2_out) *beta2_out = o.beta2;
    if (weight_decay_out) *weight_decay_out = o.weight_decay;
    return 0;
  });
}
