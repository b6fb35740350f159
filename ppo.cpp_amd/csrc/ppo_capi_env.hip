// ppo_capi_env.hip — the device env side of the C-ABI (include/ppo_synth_env.h, include/ppo_env_wrappers.h):
// the synthetic device envs (psyn_*), the PPO trainer's wrapper chain on the device (pwrap_*), and the two
// calls that run an agent against a device env without leaving the GPU, ppo_rollout_synth and
// ppo_evaluate_synth.
#include "ppo_capi_internal.hpp"
#include "ppo_env_kinds.hpp"

// ------------------------------------------------------------------------------------------
// synthetic device env
// ------------------------------------------------------------------------------------------
extern "C" int psyn_create(int E, int O, int A, psyn_t** out) {
  if (!out || E <= 0 || O <= 0 || A <= 0) return fail("psyn_create: bad arguments");
  if (O > PSYN_MAXO) return fail("psyn_create: obs_dim > 384 is not supported by the device env");
  psyn_t* env = new psyn_t();
  memset(&env->a, 0, sizeof(env->a));
  (void)hipGetDevice(&env->device);
  SynthArgs& a = env->a;
  a.E = E; a.O = O; a.A = A;
  int rc = 0;
  rc |= dmalloc(&a.q, (size_t)E * O);
  rc |= dmalloc(&a.t, E);
  rc |= dmalloc(&a.autoreset, E);
  rc |= dmalloc(&a.rseed, E);
  rc |= dmalloc(&a.rcount, E);
  rc |= dmalloc(&a.ep_ret, E);
  rc |= dmalloc(&a.ep_len, E);
  rc |= dmalloc(&a.fin_ret, E);
  rc |= dmalloc(&a.fin_len, E);
  rc |= dmalloc(&a.fin_cnt, E);
  if (rc) {
    psyn_destroy(env);
    return -2;
  }
  HIP_TRY(hipDeviceSynchronize());
  *out = env;
  return 0;
}

// every check comes before the first HIP call (psyn_create's hipGetDevice)
extern "C" int psyn_create_env(const char* env_id, int E, psyn_t** out) {
  if (!env_id || !out) return fail("psyn_create_env: null argument");
  if (E <= 0) return fail("psyn_create_env: num_envs must be positive");
  const std::string id = env_id;
  if (id == "SyntheticCheetah-v0") return psyn_create(E, 17, 6, out);
  const EnvKindRow* row = nullptr;
  for (const EnvKindRow& r : kEnvKinds)
    if (id == r.env_id) row = &r;
  if (!row)
    return fail("psyn_create_env: unknown env_id " + id +
                " (Pendulum-v1, SyntheticCheetah-v0), CartPoleContinuous-v1, ReacherPlanar-v0, QuadrotorHover-v0, AcrobotContinuous-v1");
  if (int rc = psyn_create(E, row->O, row->A, out)) return rc;
  (*out)->a.kind = row->kind;
  (*out)->act_lo = row->act_lo;
  (*out)->act_hi = row->act_hi;
  // the unused state slots of q [E, O] are defined from the start (the persistent kernels carry them along)
  if (row->zero_q) HIP_TRY(hipMemset((*out)->a.q, 0, sizeof(float) * (size_t)E * row->O));
  return 0;
}

// the cheetah (no row in kEnvKinds) truncates after CHEE_MAX_STEPS steps and never terminates
static int psyn_max_steps(const psyn_t* env) {
  const EnvKindRow* row = env_kind_row_of(env->a.kind);
  return row ? row->max_steps : CHEE_MAX_STEPS;
}
static bool psyn_terminates(const psyn_t* env) {
  const EnvKindRow* row = env_kind_row_of(env->a.kind);
  return row && row->terminates;
}
static std::string psyn_kind_name(int kind) {
  const EnvKindRow* row = env_kind_row_of(kind);
  return row ? std::string(row->kind_name) + " (" + row->env_id + ")" : "PSYN_CHEETAH";
}

extern "C" int psyn_env_info(const psyn_t* env, int* kind, int* obs_dim, int* act_dim, int* max_steps) {
  if (!env) return fail("psyn_env_info: null env");
  if (kind) *kind = env->a.kind;
  if (obs_dim) *obs_dim = env->a.O;
  if (act_dim) *act_dim = env->a.A;
  if (max_steps) *max_steps = psyn_max_steps(env);
  return 0;
}

extern "C" int psyn_destroy(psyn_t* env) {
  if (!env) return 0;
  SynthArgs& a = env->a;
  void* ptrs[] = {a.q, a.t, a.autoreset, a.rseed, a.rcount, a.ep_ret, a.ep_len, a.fin_ret, a.fin_len, a.fin_cnt};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (env->host_stats) (void)hipHostFree(env->host_stats);
  if (env->stats_ev) (void)hipEventDestroy(env->stats_ev);
  delete env;
  return 0;
}

extern "C" int psyn_reset(psyn_t* env, int seed, float* obs, float* done, void* stream) {
  if (!env || !obs) return fail("psyn_reset: null argument");
  launch_synth_reset(env->a, seed, obs, done, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int psyn_step(psyn_t* env, int e0, int e1, const float* act, float lo, float hi, float* obs, float* reward,
                         float* done, void* stream) {
  if (!env || !act || !obs || !reward || !done) return fail("psyn_step: null argument");
  if (e0 < 0 || e1 > env->a.E || e0 >= e1) return fail("psyn_step: env range out of bounds");
  launch_synth_step(env->a, e0, e1, act, lo, hi, obs, reward, done, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return 0;
}

// k_rollout_w's value pass over the n = T E stored rows: k_values_w from this many rows on, k_act3's critic
// workgroups (ppo_get_value) below; the values are the same bits either way. Measured on an MI355X, HIP
// events per launch, medians of three alternating repetitions (profiles/values_wide/values_wide_timing.txt),
// k_values_w / k_act3: n = 2 048: 31.4 / 21.6 us, 4 096: 32.6 / 22.4 us, 8 192: 33.9 / 40.4 us, 16 384: 60.8 /
// 76.6 us, 32 768: 110.8 / 144.3 us, 524 288: 1 539 / 2 156 us. Up to 4 096 rows k_act3's 16-row workgroups
// are one round of the 256 CUs, and k_values_w's 32-row passes leave CUs idle after a longer prologue (W2
// into registers); from 8 192 rows on every repetition of k_values_w beat every one of k_act3. Between the
// two sizes nothing was measured, so the threshold is the smallest size at which it won.
constexpr long kValuesWMinRows = 8192;

// the persistent rollout's arguments that come from the context; the caller adds the env and its state
static RolloutArgs base_rollout(ppo_t* c) {
  RolloutArgs r;
  memset(&r, 0, sizeof(r));
  r.P = c->P;
  r.K = c->K;
  r.WSW = c->WSW[1];
  r.E = c->cfg.num_envs;
  r.T = c->cfg.num_steps;
  r.step0 = c->iteration * (long)c->cfg.num_steps;
  r.seed = c->cfg.seed;
  r.rank = c->rank;
  r.s_obs = c->buf[PPO_BUF_OBS];
  r.s_actions = c->buf[PPO_BUF_ACTIONS];
  r.s_logp = c->buf[PPO_BUF_LOGPROBS];
  r.s_dones = c->buf[PPO_BUF_DONES];
  r.s_rewards = c->buf[PPO_BUF_REWARDS];
  r.variant = c->plan.rollout_kernel;
  return r;
}

// One full device-resident rollout (ppo:387-434 with the env behind the gymcpp boundary replaced by
// the synthetic device env): T x {agent act + store, env step, reward store}. next_obs / next_done
// carry the env state across iterations exactly like the reference's next_obs / next_done tensors.
extern "C" int ppo_rollout_synth(ppo_t* c, psyn_t* env, float* next_obs, float* next_done, float* act_scratch,
                                 float* rew_scratch) {
  if (!c || !env || !next_obs || !next_done || !act_scratch || !rew_scratch) return fail("ppo_rollout_synth: null argument");
  const int E = c->cfg.num_envs;
  if (env->a.E != E || env->a.O != c->K.O || env->a.A != c->K.A) return fail("ppo_rollout_synth: env shape mismatch");
  const float lo = env->act_lo, hi = env->act_hi;
  // the AC kernel has no wrapper chain (the AC trainer's envs carry none, ac:50-53); the PPO kernel
  // runs k_act4's arithmetic (the per-step path's kernel at O >= 112, or with act_kernel=4)
  const bool persistent = c->rollout_mode == PPO_ROLLOUT_AUTO && rollout_supported(c->K) == 0 &&
                          (c->K.kind == PPO_NET_TANH_NORMAL || !env->a.w.on);
  if (c->plan.rollout_kernel == 3 && !persistent)  // an explicit kernel that cannot run is an error, not a silent per-step path
    return fail("ppo_rollout_synth: rollout_kernel=split needs the persistent rollout: at most 8 actions, no device env wrappers");
  // the AC agent at Humanoid width (k_rollout_w: OP = 384, 17 <= A <= 24, the cheetah-shaped env, no
  // wrappers): one persistent launch for all T steps, then the log-probs and the critic over the stored rows
  if (c->rollout_mode == PPO_ROLLOUT_AUTO && rollout_w_supported(c->K) == 0 && !env->a.w.on && env->a.kind == PSYN_CHEETAH) {
    const long n = (long)E * c->cfg.num_steps;
    RolloutArgs r = base_rollout(c);
    r.next_obs = next_obs;
    r.next_done = next_done;
    r.env = env->a;
    r.lo = lo;
    r.hi = hi;
    if (!c->beta_store && dmalloc(&c->beta_store, (size_t)n * c->K.A * 3)) return -2;
    r.s_beta = c->beta_store;
    {
      ProfScope ps(c, PK_ROLLOUT, c->stream);
      if (const int lrc = launch_rollout_w(r, c->stream))
        return lrc == -6 ? lrc : fail("ppo_rollout_synth: rollout kernel launch failed");  // -6: launch_rollout_w's message
      launch_beta_logp(r.s_beta, c->buf[PPO_BUF_LOGPROBS], n, c->K.A, c->stream);
    }
    c->values_pending.store(0);  // every stored row's value comes from this pass
    // the critic of the stored rows: k_values_w (run_values), bitwise k_act3's critic workgroups, which the
    // per-step path's values come from; a row's value does not depend on the rows beside it
    if (n >= kValuesWMinRows) {
      if (run_values(c, c->buf[PPO_BUF_OBS], c->buf[PPO_BUF_VALUES], n, c->stream) != 0)
        return fail("ppo_rollout_synth: values kernel launch failed");
    } else if (int rc = ppo_get_value(c, (int)n, c->buf[PPO_BUF_OBS], c->buf[PPO_BUF_VALUES], c->stream)) {
      return rc;
    }
    HIP_TRY(hipGetLastError());
    c->rollout_path = 4;
    return 0;
  }
  if (persistent) {
    // one persistent launch for all T steps (k_rollout), then the critic over the stored rows
    RolloutArgs r = base_rollout(c);
    r.next_obs = next_obs;
    r.next_done = next_done;
    r.env = env->a;
    r.lo = lo;
    r.hi = hi;
    if (c->K.kind == PPO_NET_LN_BETA) {  // Beta log-probs after the rollout (off the env's path)
      if (!c->beta_store && dmalloc(&c->beta_store, (size_t)E * c->cfg.num_steps * c->K.A * 3)) return -2;
      r.s_beta = c->beta_store;
    }
    {
      ProfScope ps(c, PK_ROLLOUT, c->stream);
      if (const int lrc = launch_rollout(r, c->stream))
        return fail(lrc == -4 ? std::string("ppo_rollout_synth: rollout_kernel=valu steps the synthetic cheetah only; this env's "
                                            "kind is ") + psyn_kind_name(env->a.kind) + ": use rollout_kernel=auto or mfma"
                    : lrc == -3 ? "ppo_rollout_synth: rollout_kernel=valu needs the LayerNorm-Beta agent, O <= 32 and no "
                                "device env wrappers"
                    : lrc == -5 ? "ppo_rollout_synth: rollout_kernel=split needs the LayerNorm-Beta agent, O <= 32, at most "
                                "8 actions and no device env wrappers"
                              : "ppo_rollout_synth: rollout kernel launch failed");
      if (r.s_beta) launch_beta_logp(r.s_beta, c->buf[PPO_BUF_LOGPROBS], (long)E * c->cfg.num_steps, c->K.A, c->stream);
    }
    c->values_pending.store(0);  // every stored row's value comes from this pass
    if (run_values(c, c->buf[PPO_BUF_OBS], c->buf[PPO_BUF_VALUES], (long)E * c->cfg.num_steps, c->stream) != 0)
      return fail("ppo_rollout_synth: values kernel launch failed");
    HIP_TRY(hipGetLastError());
    c->rollout_path = c->K.kind == PPO_NET_LN_BETA ? 1 : 3;
    return 0;
  }
  for (int t = 0; t < c->cfg.num_steps; ++t) {
    int rc = ppo_rollout_act(c, t, 0, E, next_obs, next_done, act_scratch, nullptr);
    if (rc) return rc;
    {
      ProfScope ps(c, PK_SYNTH, c->stream);
      // the env's reward output IS rewards[t] of the rollout storage (ppo:406) — no extra copy
      launch_synth_step(env->a, 0, E, act_scratch, lo, hi, next_obs, c->buf[PPO_BUF_REWARDS] + (size_t)t * E,
                        next_done, c->stream);
    }
  }
  if (int rc = flush_values(c, c->stream)) return rc;  // the rollout's values, as the persistent path leaves them
  HIP_TRY(hipGetLastError());
  c->rollout_path = 2;
  return 0;
}

extern "C" int ppo_rollout_info(const ppo_t* c, char* buf, int len) {
  if (!c || !buf || len <= 0) return fail("ppo_rollout_info: null argument");
  snprintf(buf, (size_t)len, "rollout=%s",
           c->rollout_path == 1 ? "k_rollout" : c->rollout_path == 2 ? "per_step" : c->rollout_path == 3 ? "k_rollout4"
           : c->rollout_path == 4 ? "k_rollout_w" : "none");
  return 0;
}

// the persistent evaluation's arguments that come from the context; the caller adds the env, the chunk
// and the event buffer
static EvalArgs base_eval(ppo_t* c) {
  EvalArgs a;
  memset(&a, 0, sizeof(a));
  a.P = c->P;
  a.K = c->K;
  a.WSW = c->WSW[1];
  a.seed = c->cfg.seed;
  a.rank = c->rank;
  return a;
}

// Policy evaluation on the device env (ac:965-1001 with num_eval_envs = 1; ppo:589-626 with all envs).
// Chunks of env steps run on the context stream, either as one persistent launch each (k_eval, or k_eval_w
// at Humanoid width; with mode = 2 also k_eval4, the PPO agent's) or as chunk x {act, psyn_step, k_eval_record}; after each chunk one read-out of the event buffer (its
// counter in the first record) decides whether another chunk is needed. Both paths produce the same
// events bit for bit, and the kept list depends on the events only (eval_select), not on the chunks.
extern "C" int ppo_evaluate_synth(ppo_t* c, psyn_t* env, const ppo_eval_config* cfg, float* returns_host,
                                  int* lengths_host, int cap, int* n_out, long* env_steps_out) {
  if (!c || !env || !cfg || !returns_host || !lengths_host || !n_out || !env_steps_out)
    return fail("ppo_evaluate_synth: null argument");
  const int E = env->a.E, O = env->a.O, A = env->a.A, nE = cfg->num_eval_envs, runs = cfg->num_eval_runs;
  if (runs <= 0) return fail("ppo_evaluate_synth: num_eval_runs must be positive");
  if (nE < 1 || nE > E) return fail("ppo_evaluate_synth: num_eval_envs must be in [1, " + std::to_string(E) + "]");
  if ((long)cap < (long)runs + nE - 1)
    return fail("ppo_evaluate_synth: cap must be at least num_eval_runs + num_eval_envs - 1 = " + std::to_string((long)runs + nE - 1));
  if (cfg->sample_type == PPO_GIVEN) return fail("ppo_evaluate_synth: PPO_GIVEN is not an evaluation sample type");
  if (cfg->sample_type < 0 || cfg->sample_type > PPO_ROACH || (cfg->sample_type == PPO_ROACH && c->K.kind != PPO_NET_LN_BETA))
    return fail("Unsupported sample type used. Sample type: " + std::to_string(cfg->sample_type));
  if (O != c->K.O || A != c->K.A) return fail("ppo_evaluate_synth: env shape mismatch");
  if (cfg->chunk_steps < 0 || cfg->mode < 0 || cfg->mode > 2) return fail("ppo_evaluate_synth: bad chunk_steps / mode");
  // the path (ppo_t::eval_path): auto takes k_eval or k_eval_w where one applies and the per-step
  // launches otherwise; mode = 2 takes a persistent kernel, k_eval, k_eval_w or k_eval4, or refuses
  int path = 2;
  if (cfg->mode != 1 && eval_supported(c->K) == 0 && !env->a.w.on) path = 1;
  else if (cfg->mode != 1 && eval_w_supported(c->K) == 0 && !env->a.w.on && env->a.kind == PSYN_CHEETAH) path = 4;
  else if (cfg->mode == 2 && eval4_supported(c->K) == 0) path = 3;
  else if (cfg->mode == 2)
    return fail(std::string("ppo_evaluate_synth: mode = 2 (persistent) has no kernel for the ") +
                (c->K.kind == PPO_NET_LN_BETA ? "LayerNorm-Beta" : "tanh-Normal") + " agent at H = " + std::to_string(c->K.H) +
                ", OP = " + std::to_string(c->K.OP) + ", A = " + std::to_string(A) +
                (env->a.w.on ? " on an env with the wrapper chain" : "") +
                ": k_eval serves LayerNorm-Beta, H = 256, OP <= 32, A <= 8 without wrappers; k_eval4 tanh-Normal, H = 64, "
                "OP in {16, 32, 112, 384}, A <= 32; use mode = 0 or 1");
  // an env that terminates can finish an episode every other step, so its chunks are shorter by
  // default (the event buffer below is sized for the worst case)
  const bool terminates = psyn_terminates(env);
  const int chunk = cfg->chunk_steps > 0 ? cfg->chunk_steps : (terminates ? 512 : 4096);
  // the env truncates after max_steps (the cheetah CHEE_MAX_STEPS, Pendulum 200) steps and resets on the next one: an env
  // finishes at most one episode per max_steps + 1 steps, which bounds the events of a chunk (an
  // overflow is still detected). CartPoleContinuous-v1 and QuadrotorHover-v0 terminate: an episode is
  // at least one step and the reset step after it, so an env finishes at most one episode per 2 steps.
  const int min_period = terminates ? 2 : psyn_max_steps(env) + 1;
  const long devcap = (long)nE * (chunk / min_period + 2);
  hipStream_t s = c->stream;
  struct Scratch {
    char* p = nullptr;
    ~Scratch() { if (p) (void)hipFree(p); }
  } scratch;
  const size_t nfl = (size_t)E * O + 2 * (size_t)E + (size_t)nE * A;
  const size_t ev_off = (nfl * sizeof(float) + 15) / 16 * 16;
  const size_t ev_bytes = (size_t)(devcap + 1) * sizeof(EvalEvent);  // record 0 holds the counter
  HIP_TRY(hipMalloc((void**)&scratch.p, ev_off + ev_bytes));
  float* d_obs = reinterpret_cast<float*>(scratch.p);
  float* d_done = d_obs + (size_t)E * O;
  float* d_rew = d_done + E;
  float* d_act = d_rew + E;
  EvalEvent* d_ev = reinterpret_cast<EvalEvent*>(scratch.p + ev_off);
  unsigned* d_count = reinterpret_cast<unsigned*>(d_ev);
  const float lo = env->act_lo, hi = env->act_hi;
  launch_synth_reset(env->a, cfg->eval_seed, d_obs, d_done, s);
  std::vector<EvalEvent> all, host((size_t)devcap + 1);
  long long k = 0, stop = 0;
  size_t keep = 0;
  while (keep == 0) {
    HIP_TRY(hipMemsetAsync(d_ev, 0, sizeof(EvalEvent), s));
    if (path != 2) {
      EvalArgs a = base_eval(c);
      a.nE = nE;
      a.T = chunk;
      a.step0 = cfg->step0 + (long)k;
      a.k0 = k;
      a.mode = cfg->sample_type;
      a.obs = d_obs;
      a.env = env->a;
      a.lo = lo;
      a.hi = hi;
      a.ev = d_ev + 1;
      a.count = d_count;
      a.cap = (int)devcap;
      if ((path == 1 ? launch_eval(a, s) : path == 4 ? launch_eval_w(a, s) : launch_eval4(a, s)) != 0)
        return fail("ppo_evaluate_synth: evaluation kernel launch failed");
    } else {
      for (int t = 0; t < chunk; ++t) {
        if (int rc = ppo_get_action_and_value(c, nE, d_obs, cfg->sample_type, nullptr, 0, cfg->step0 + (long)(k + t), d_act,
                                              nullptr, nullptr, nullptr, s))
          return rc;
        launch_synth_step(env->a, 0, nE, d_act, lo, hi, d_obs, d_rew, d_done, s);
        launch_eval_record(env->a, d_done, nE, k + t, d_ev + 1, d_count, (int)devcap, s);
      }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host.data(), d_ev, ev_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const unsigned got = *reinterpret_cast<const unsigned*>(host.data());
    if ((long)got > devcap) return fail("ppo_evaluate_synth: event buffer overflow");
    all.insert(all.end(), host.begin() + 1, host.begin() + 1 + got);
    k += chunk;
    keep = eval_select(all, runs, &stop);
  }
  for (size_t i = 0; i < keep; ++i) {
    returns_host[i] = all[i].ret;
    lengths_host[i] = all[i].len;
  }
  *n_out = (int)keep;
  *env_steps_out = (long)stop + 1;
  c->eval_path = path;
  return 0;
}

extern "C" int ppo_eval_info(const ppo_t* c, char* buf, int len) {
  if (!c || !buf || len <= 0) return fail("ppo_eval_info: null argument");
  snprintf(buf, (size_t)len, "eval=%s",
           c->eval_path == 1 ? "k_eval" : c->eval_path == 2 ? "per_step" : c->eval_path == 3 ? "k_eval4" : c->eval_path == 4 ? "k_eval_w" : "none");
  return 0;
}

extern "C" int psyn_episode_stats_begin(psyn_t* env, void* stream) {
  if (!env) return fail("null env");
  const int E = env->a.E;
  hipStream_t s = (hipStream_t)stream;
  if (!env->host_stats) {
    HIP_TRY(hipHostMalloc(&env->host_stats, sizeof(float) * 3 * E));
    HIP_TRY(hipEventCreateWithFlags(&env->stats_ev, hipEventDisableTiming));
  }
  float* src[3] = {env->a.fin_ret, env->a.fin_len, env->a.fin_cnt};
  for (int k = 0; k < 3; ++k) {
    HIP_TRY(hipMemcpyAsync(env->host_stats + (size_t)k * E, src[k], sizeof(float) * E, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(src[k], 0, sizeof(float) * E, s));
  }
  HIP_TRY(hipEventRecord(env->stats_ev, s));
  return 0;
}

extern "C" int psyn_episode_stats_end(psyn_t* env, float* sr, float* sl, float* sc) {
  if (!env || !env->stats_ev) return fail("psyn_episode_stats_end: no read-out pending");
  HIP_TRY(hipEventSynchronize(env->stats_ev));
  const int E = env->a.E;
  double R = 0, Lsum = 0, N = 0;
  const float* h = env->host_stats;
  for (int i = 0; i < E; ++i) { R += h[i]; Lsum += h[E + i]; N += h[2 * E + i]; }
  if (sr) *sr = (float)R;
  if (sl) *sl = (float)Lsum;
  if (sc) *sc = (float)N;
  return 0;
}

extern "C" int psyn_episode_stats(psyn_t* env, float* sr, float* sl, float* sc) {
  if (!env) return fail("null env");
  const int E = env->a.E;
  std::vector<float> r(E), l(E), n(E);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(r.data(), env->a.fin_ret, sizeof(float) * E, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(l.data(), env->a.fin_len, sizeof(float) * E, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n.data(), env->a.fin_cnt, sizeof(float) * E, hipMemcpyDeviceToHost));
  double R = 0, Lsum = 0, N = 0;
  for (int i = 0; i < E; ++i) { R += r[i]; Lsum += l[i]; N += n[i]; }
  HIP_TRY(hipMemset(env->a.fin_ret, 0, sizeof(float) * E));
  HIP_TRY(hipMemset(env->a.fin_len, 0, sizeof(float) * E));
  HIP_TRY(hipMemset(env->a.fin_cnt, 0, sizeof(float) * E));
  HIP_TRY(hipDeviceSynchronize());
  if (sr) *sr = (float)R;
  if (sl) *sl = (float)Lsum;
  if (sc) *sc = (float)N;
  return 0;
}

extern "C" int psyn_set_action_space(psyn_t* env, float lo, float hi) {
  if (!env || !(lo < hi)) return fail("psyn_set_action_space: bad arguments");
  env->act_lo = lo;
  env->act_hi = hi;
  return 0;
}

extern "C" int psyn_action_space(const psyn_t* env, float* lo, float* hi) {
  if (!env || !lo || !hi) return fail("psyn_action_space: null argument");
  *lo = env->act_lo;
  *hi = env->act_hi;
  return 0;
}

// ------------------------------------------------------------------------------------------
// PPO env wrapper chain on the device (include/ppo_env_wrappers.h)
// ------------------------------------------------------------------------------------------
extern "C" int pwrap_create(int E, int O, float gamma, pwrap_t** out) {
  if (!out || E <= 0 || O <= 0) return fail("pwrap_create: bad arguments");
  pwrap_t* p = new pwrap_t();
  p->E = E;
  p->O = O;
  const size_t n = 2 * (size_t)E * O + 5 * (size_t)E;
  if (dmalloc(&p->state, n)) {
    delete p;
    return -2;
  }
  std::vector<float> h(n, 0.0f);  // mean 0, var 1, obs count 1e-4; reward mean 0, var 1, acc 0, count 1e-8
  for (size_t k = (size_t)E * O; k < 2 * (size_t)E * O; ++k) h[k] = 1.0f;
  float* tail = h.data() + 2 * (size_t)E * O;
  for (int e = 0; e < E; ++e) {
    tail[e] = 1e-4f;
    tail[2 * E + e] = 1.0f;
    tail[4 * E + e] = 1e-8f;
  }
  HIP_TRY(hipMemcpy(p->state, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
  WrapArgs& w = p->w;
  w.om = p->state;
  w.ov = p->state + (size_t)E * O;
  w.ocount = p->state + 2 * (size_t)E * O;
  w.rmean = w.ocount + E;
  w.rvar = w.rmean + E;
  w.racc = w.rvar + E;
  w.rcount = w.racc + E;
  w.gamma = gamma;
  w.on = 1;
  *out = p;
  return 0;
}

extern "C" int pwrap_destroy(pwrap_t* p) {
  if (!p) return 0;
  if (p->state) (void)hipFree(p->state);
  delete p;
  return 0;
}

extern "C" int pwrap_reset(pwrap_t* p, int e0, int e1, float* obs, void* stream) {
  if (!p || !obs) return fail("pwrap_reset: null argument");
  if (e0 < 0 || e1 > p->E || e0 >= e1) return fail("pwrap_reset: env range out of bounds");
  launch_wrap_step(p->w, p->O, e0, e1, obs, nullptr, nullptr, nullptr, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int pwrap_step(pwrap_t* p, int e0, int e1, float* obs, float* reward, const float* term,
                          const float* is_reset, void* stream) {
  if (!p || !obs || !reward) return fail("pwrap_step: null argument");
  if (e0 < 0 || e1 > p->E || e0 >= e1) return fail("pwrap_step: env range out of bounds");
  launch_wrap_step(p->w, p->O, e0, e1, obs, reward, term, is_reset, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int pwrap_read_state(pwrap_t* p, float* host, long n) {
  if (!p || !host) return fail("pwrap_read_state: null argument");
  if (n != 2L * p->E * p->O + 5L * p->E) return fail("pwrap_read_state: size mismatch");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host, p->state, n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int psyn_attach_wrappers(psyn_t* env, pwrap_t* p) {
  if (!env) return fail("psyn_attach_wrappers: null env");
  if (!p) {
    env->a.w = WrapArgs{};
    return 0;
  }
  if (p->E != env->a.E || p->O != env->a.O) return fail("psyn_attach_wrappers: shape mismatch");
  env->a.w = p->w;
  return 0;
}

extern "C" int ppo_set_rollout_mode(ppo_t* c, int mode) {
  if (!c) return fail("null ctx");
  if (mode != PPO_ROLLOUT_AUTO && mode != PPO_ROLLOUT_PER_STEP) return fail("ppo_set_rollout_mode: bad mode");
  c->rollout_mode = mode;
  return 0;
}
