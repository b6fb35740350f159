// ppo_capi.hip — C-ABI of libppo_hip.so (include/ppo_hip.h): the context and the agent calls.
//
// Host runtime around the gfx950 kernels: device memory for the agent (packed params, grads,
// Adam moments), the [T, E, *] rollout storage and minibatch scratch, allocated by ppo_create_ex from
// the kernel plan (ppo_capi_plan.hip); act, values, GAE, parameter / Adam / snapshot I/O, profiling.
// The update is in ppo_capi_update.hip, the communicator in ppo_capi_comm.hip, the device envs in
// ppo_capi_env.hip. Everything runs asynchronously on the context stream; the only host
// synchronisation in an update is the optional stats read-back at its end.
#include <dlfcn.h>
#include <link.h>
#include <unistd.h>

#include "ppo_capi_internal.hpp"

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;
int ppo_fail(const std::string& msg, int code) {
  g_err = msg;
  return code;
}

extern "C" const char* ppo_last_error(void) { return g_err.c_str(); }

// ------------------------------------------------------------------------------------------
// one HIP runtime per process
// ------------------------------------------------------------------------------------------
// libppo_hip.so links /opt/rocm's libamdhip64.so.7. A PyTorch-ROCm wheel bundles its own copy and
// its libraries ask for it as "libamdhip64.so"; if libppo_hip.so is loaded first, `import torch`
// then maps a second HIP runtime, and the two tear each other down at exit (free(): invalid
// pointer, exit 134). Every runtime-initialising entry point checks for that and fails with a
// clear message; the first failed check also installs an exit guard that ends the process with
// status 70 before either runtime's teardown runs. The guard is permanent for the process (a host
// that handles the -4 still exits 70: its teardown would crash otherwise); it flushes every stdio
// stream first.
static int hip_runtime_paths(std::vector<std::string>* out) {
  out->clear();
  dl_iterate_phdr(
      [](struct dl_phdr_info* info, size_t, void* data) -> int {
        auto* v = static_cast<std::vector<std::string>*>(data);
        const char* name = info->dlpi_name;
        if (!name || !strstr(name, "libamdhip64.so")) return 0;
        char buf[4096];
        std::string path = realpath(name, buf) ? std::string(buf) : std::string(name);
        if (std::find(v->begin(), v->end(), path) == v->end()) v->push_back(path);
        return 0;
      },
      out);
  return (int)out->size();
}

static std::string g_runtime_msg;
static void runtime_exit_guard() {
  fprintf(stderr, "libppo_hip: %s -- exiting (70) before the HIP runtimes' teardown\n", g_runtime_msg.c_str());
  fflush(nullptr);  // every stdio stream (stdout, log files) before _exit skips the C library's flush
  _exit(70);
}

extern "C" int ppo_runtime_check(void) {
  std::vector<std::string> paths;
  if (hip_runtime_paths(&paths) <= 1) return 0;
  std::string msg = "two HIP runtimes are mapped in this process (";
  for (size_t i = 0; i < paths.size(); ++i) msg += (i ? ", " : "") + paths[i];
  msg += "): load libppo_hip.so after `import torch` (ppo_amd does), or do not import torch";
  static std::once_flag guard;
  std::call_once(guard, [&] {
    g_runtime_msg = msg;
    atexit(runtime_exit_guard);
  });
  return fail(msg, -4);
}

// ------------------------------------------------------------------------------------------
// per-env-id observation normalisation of the AC agent (ac:480-534)
// ------------------------------------------------------------------------------------------
#include "ppo_obs_norm.inc"

extern "C" int ppo_obs_norm(const char* env_id, const float** mean, const float** stdv, int* n) {
  if (!env_id || !mean || !stdv || !n) return fail("ppo_obs_norm: null argument");
  *mean = *stdv = nullptr;
  *n = 0;
  if (!strcmp(env_id, "HalfCheetah-v5")) return 0;  // zeros / ones (ac:510-511): identity
  if (!strcmp(env_id, "CartPoleContinuous-v1")) return 0;  // raw (x, xdot, theta, thetadot): identity
  if (!strcmp(env_id, "ReacherPlanar-v0")) return 0;       // all ten values are of order 1 or smaller: identity
  if (!strcmp(env_id, "QuadrotorHover-v0")) return 0;      // positions, a rotation matrix, speeds of order 1: identity
  for (const ObsNormEntry& e : k_obs_norm)
    if (!strcmp(env_id, e.env_id)) {
      *mean = e.mean;
      *stdv = e.std;
      *n = e.n;
      return 0;
    }
  return fail(std::string("ppo_obs_norm: env_id ") + env_id + " is not implemented.", -1);
}
extern "C" const char* ppo_version(void) { return "ppo_hip 0.1 (gfx950)"; }

// ------------------------------------------------------------------------------------------
// profiling (HIP events around the context's launches: ProfScope, ppo_capi_internal.hpp)
// ------------------------------------------------------------------------------------------
static const char* kProfNames[PK_COUNT] = {"act", "fwdbwd", "dw", "dw_l1", "colsum", "gradnorm",
                                           "adam", "gae", "perm", "adv_stats", "allreduce", "synth_env",
                                           "rollout", "values", "l1g"};

static void prof_drain(ppo_t* c) {
  std::lock_guard<std::mutex> lk(c->prof_mu);
  for (auto& p : c->pending) {
    (void)hipEventSynchronize(p.b);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, p.a, p.b);
    c->prof_ms[p.id] += ms;
    c->prof_cnt[p.id] += 1;
    c->free_events.push_back(p.a);
    c->free_events.push_back(p.b);
  }
  c->pending.clear();
}

// ------------------------------------------------------------------------------------------
// create / destroy
// ------------------------------------------------------------------------------------------
extern "C" int ppo_create(const ppo_hip_config* cfg, int device, ppo_t** out) {
  return ppo_create_ex(cfg, device, nullptr, out);
}

// Device memory of a context, sized from its kernel plan; on failure the caller destroys the context.
static int alloc_context(ppo_t* c) {
  const ppo_hip_config& cfg = c->cfg;
  const KernelPlan& kp = c->plan;
  const int H = cfg.hidden, A = cfg.act_dim, O = cfg.obs_dim, OP = c->K.OP;
  int rc = 0;
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  const size_t PS = c->K.size;
  rc |= dmalloc(&c->P, PS); rc |= dmalloc(&c->G, PS); rc |= dmalloc(&c->Am, PS); rc |= dmalloc(&c->Av, PS);
  for (int k = 0; k < 2; ++k) rc |= dmalloc(&c->W2T[k], (size_t)H * H);
  // room for the split-bf16 pieces after the fp32 copies (upd_mfma=bx6): W2 | W2^T at H = 256, W1 at 64
  for (int k = 0; k < 2; ++k) rc |= dmalloc(&c->WSW[k], (size_t)(sw_size(H, c->K.OP) + bx_region(H, c->K.OP)));
  const size_t E = cfg.num_envs, T = cfg.num_steps;
  rc |= dmalloc(&c->buf[PPO_BUF_OBS], T * E * O);
  rc |= dmalloc(&c->buf[PPO_BUF_ACTIONS], T * E * A);
  for (int b = PPO_BUF_LOGPROBS; b < PPO_BUF_COUNT; ++b)
    if (b != PPO_BUF_ACTIONS) rc |= dmalloc(&c->buf[b], T * E);
  rc |= dmalloc(&c->next_value, E);
  const int EP = cfg.update_epochs;
  rc |= dmalloc(&c->perms, (size_t)EP * c->B);
  rc |= dmalloc(&c->advstats, (size_t)2 * EP * c->nmb);
  rc |= dmalloc(&c->advsq, (size_t)EP * c->nmb);
  rc |= dmalloc(&c->advpart, (size_t)EP * c->nmb * PPO_ADV_SPLIT);
  const size_t Mr = ((size_t)c->M + 63) / 64 * 64;
  rc |= dmalloc(&c->Xn, Mr * OP + 64);
  for (int k = 0; k < 2; ++k) {
    rc |= dmalloc(&c->H1[k], Mr * H);
    rc |= dmalloc(&c->DZ1[k], Mr * H);
    rc |= dmalloc(&c->DZ2[k], Mr * H);
  }
  // one slab row per workgroup of each of the minibatch's launches; one dW partial row per chunk of each
  for (int k = 0; k < 2; ++k)
    rc |= dmalloc(&c->slab[k], (size_t)kp.msplit * std::max(kp.nblk, kp.upd_nblk) * c->sg[k].size);
  if (kp.h1_recomp)
    for (int k = 0; k < 2; ++k) rc |= dmalloc(&c->LNS[k], 2 * (size_t)c->M);
  for (int k = 0; k < 2; ++k) rc |= dmalloc(&c->dwslab[k], (size_t)kp.msplit * kp.nchunks * (H * H + H * OP));
  if (kp.upd2_split) rc |= dmalloc(&c->Z1, Mr * 128);
  rc |= dmalloc(&c->normout, 2 + PPO_LAYOUT_MAX_TENSORS + 2);
  rc |= dmalloc(&c->gnpart, (size_t)PPO_LAYOUT_MAX_TENSORS * PPO_GN_SPLIT);
  rc |= dmalloc(reinterpret_cast<float**>(&c->gs_bar), 1);
  rc |= dmalloc(&c->cs_sq, (size_t)c->K.size / 64 + 2 * PPO_MAX_SEGS + 64);
  rc |= dmalloc(reinterpret_cast<float**>(&c->cs_cnt), PPO_MAX_SEGS);
  rc |= dmalloc(&c->mbstats, (size_t)8 * EP * c->nmb);
  return rc ? -2 : 0;
}

extern "C" int ppo_create_ex(const ppo_hip_config* cfg, int device, const char* options, ppo_t** out) {
  if (!cfg || !out) return fail("ppo_create: null argument");
  CreateOptions opt;
  if (parse_create_options(options, &opt)) return -1;
  if (int rc = ppo_runtime_check()) return rc;
  ppo_layout L;
  if (ppo_layout_init(&L, cfg->net_kind, cfg->obs_dim, cfg->act_dim, cfg->hidden) != 0)
    return fail("ppo_create: bad net kind / dims");
  if (cfg->hidden != 64 && cfg->hidden != 256) return fail("ppo_create: hidden must be 64 or 256");
  if (cfg->act_dim > 20) return fail("ppo_create: act_dim > 20 not supported");
  if (cfg->num_envs <= 0 || cfg->num_steps <= 0 || cfg->num_minibatches <= 0 || cfg->update_epochs <= 0)
    return fail("ppo_create: sizes must be positive");
  const long B = (long)cfg->num_envs * cfg->num_steps;
  if (B % cfg->num_minibatches) return fail("ppo_create: num_steps*num_envs must divide by num_minibatches");
  if (B >= (1L << 31)) return fail("ppo_create: batch too large");
  {
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)  // the reference's gpu_ids.at(local_rank) throws here (ac:447)
      return fail("ppo_create: device " + std::to_string(device) + " requested but " + std::to_string(ndev) +
                  " HIP device(s) are visible");
  }
  HIP_TRY(hipSetDevice(device));
  // every decision, and every refusal of a configuration, before anything exists
  const PackedLayout K = make_packed(L);
  const int H = cfg->hidden, A = cfg->act_dim;
  const SmallGradLayout sg[2] = {make_sg(H, 1, A), make_sg(H, cfg->net_kind == PPO_NET_LN_BETA ? 2 * A : A, A)};
  KernelPlan plan;
  if (int rc = plan_kernels(*cfg, K, sg, opt, &plan)) return rc;
  ppo_t* c = new ppo_t();
  c->cfg = *cfg;
  c->device = device;
  c->L = L;
  c->K = K;
  c->sg[0] = sg[0];
  c->sg[1] = sg[1];
  c->B = B;
  c->nmb = cfg->num_minibatches;
  c->M = (int)(B / cfg->num_minibatches);
  c->rank = cfg->rank;
  c->world = 1;  // statistics and collectives span the communicator attached later (ppo_comm_init*)
  c->plan = plan;
  c->rollout_mode = opt.rollout;
  // from here on a failure has one way out
  int rc = alloc_context(c);
  if (rc == 0 && !c->plan.no_update && fwdbwd_set_lds(c->K, c->plan.lds_bytes) != 0) {
    (void)hipGetLastError();  // the refusal is reported here: the next call must not find the attribute call's error
    rc = fail("ppo_create: cannot set LDS size for the fused update kernel");
  }
  // update=off: an update form the planner probed may have been refused its LDS attribute; no kernel of
  // this context launches it, and the next call must not find that error
  if (rc == 0 && c->plan.no_update) (void)hipGetLastError();
  if (rc == 0) rc = [] { HIP_TRY(hipDeviceSynchronize()); return 0; }();
  if (rc != 0) {
    ppo_destroy(c);  // leaves the reason (ppo_last_error) as it is
    return rc;
  }
  build_update_plan(c);
  *out = c;
  return 0;
}

extern "C" int ppo_destroy(ppo_t* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  prof_drain(c);
  for (auto e : c->free_events) (void)hipEventDestroy(e);
  float* ptrs[] = {c->P, c->G, c->Am, c->Av, c->W2T[0], c->W2T[1], c->WSW[0], c->WSW[1], c->next_value, c->advstats, c->advsq, c->Xn, c->Z1,
                   c->normout, c->gnpart, c->mbstats, c->beta_store, reinterpret_cast<float*>(c->gs_bar), c->cs_sq,
                   reinterpret_cast<float*>(c->cs_cnt)};
  for (float* p : ptrs)
    if (p) (void)hipFree(p);
  for (int b = 0; b < PPO_BUF_COUNT; ++b)
    if (c->buf[b]) (void)hipFree(c->buf[b]);
  for (int k = 0; k < 2; ++k) {
    float* q[] = {c->H1[k], c->DZ1[k], c->DZ2[k], c->slab[k], c->LNS[k]};
    for (float* p : q)
      if (p) (void)hipFree(p);
  }
  for (int k = 0; k < 4; ++k)
    if (c->dwslab[k]) (void)hipFree(c->dwslab[k]);
  if (c->perms) (void)hipFree(c->perms);
  if (c->upd_exec) (void)hipGraphExecDestroy(c->upd_exec);
  if (c->sched) (void)hipFree(c->sched);
  for (int i = 0; i < 2; ++i) {
    if (c->sched_host[i]) (void)hipHostFree(c->sched_host[i]);
    if (c->sched_ev[i]) (void)hipEventDestroy(c->sched_ev[i]);
  }
  if (c->advpart) (void)hipFree(c->advpart);
  comm_detach(c);
  if (c->snap) (void)hipFree(c->snap);
  if (c->snap_ev) (void)hipEventDestroy(c->snap_ev);
  if (c->snap_stream) (void)hipStreamDestroy(c->snap_stream);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

extern "C" int ppo_get_layout(const ppo_t* c, ppo_layout* out) {
  if (!c || !out) return fail("ppo_get_layout: null argument");
  *out = c->L;
  return 0;
}
extern "C" void* ppo_stream(ppo_t* c) { return c ? (void*)c->stream : nullptr; }
extern "C" long ppo_iteration(const ppo_t* c) { return c ? c->iteration : -1; }
extern "C" int ppo_set_iteration(ppo_t* c, long it) {
  if (!c) return fail("null ctx");
  c->iteration = it;
  return 0;
}
#ifdef PPO_DIAG
// diagnostic build only (not part of the C-ABI header): internal device buffers by name
// ("beta_store": the AC rollout's (alpha, beta, sample) per (t, env, action); scripts/debug_rollout_v.py)
extern "C" float* ppo_debug_buffer(ppo_t* c, const char* name) {
  if (!c || !name) return nullptr;
  if (!strcmp(name, "beta_store")) return c->beta_store;
  return nullptr;
}
#endif
extern "C" float* ppo_buffer(ppo_t* c, int which) {
  if (!c || which < 0 || which >= PPO_BUF_COUNT) return nullptr;
  return c->buf[which];
}

// ------------------------------------------------------------------------------------------
// parameters / optimizer state
// ------------------------------------------------------------------------------------------
int refresh_weight_copies(ppo_t* c) {
  for (int k = 0; k < 2; ++k) launch_transpose(c->P + c->K.tr[k].W2, c->W2T[k], c->K.H, c->stream);
  for (int k = 0; k < 2; ++k)
    launch_swizzle(c->P + c->K.tr[k].W1, c->P + c->K.tr[k].W2, c->WSW[k], c->K.H, c->K.OP, c->plan.upd_bx, c->stream);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int ppo_load_params(ppo_t* c, const float* host, long n) {
  if (!c || !host) return fail("ppo_load_params: null argument");
  if (n != c->L.P) return fail("ppo_load_params: expected " + std::to_string(c->L.P) + " floats");
  HIP_TRY(hipSetDevice(c->device));
  std::vector<float> packed(c->K.size);
  pack_params(c->K, c->L, host, packed.data());
  HIP_TRY(hipMemcpyAsync(c->P, packed.data(), sizeof(float) * c->K.size, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->Am, 0, sizeof(float) * c->K.size, c->stream));
  HIP_TRY(hipMemsetAsync(c->Av, 0, sizeof(float) * c->K.size, c->stream));
  c->adam_step = 0;
  if (refresh_weight_copies(c)) return -2;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int ppo_save_params(ppo_t* c, float* host, long n) {
  if (!c || !host) return fail("ppo_save_params: null argument");
  if (n != c->L.P) return fail("ppo_save_params: expected " + std::to_string(c->L.P) + " floats");
  HIP_TRY(hipSetDevice(c->device));
  std::vector<float> packed(c->K.size);
  HIP_TRY(hipMemcpyAsync(packed.data(), c->P, sizeof(float) * c->K.size, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  unpack_params(c->K, c->L, packed.data(), host);
  return 0;
}

extern "C" int ppo_save_adam(ppo_t* c, float* m_host, float* v_host, long n, long* step) {
  if (!c) return fail("null ctx");
  if (n != c->L.P) return fail("ppo_save_adam: size mismatch");
  std::vector<float> pm(c->K.size), pv(c->K.size);
  HIP_TRY(hipMemcpyAsync(pm.data(), c->Am, sizeof(float) * c->K.size, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(pv.data(), c->Av, sizeof(float) * c->K.size, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (m_host) unpack_params(c->K, c->L, pm.data(), m_host);
  if (v_host) unpack_params(c->K, c->L, pv.data(), v_host);
  if (step) *step = c->adam_step;
  return 0;
}

extern "C" int ppo_load_adam(ppo_t* c, const float* m_host, const float* v_host, long n, long step) {
  if (!c || !m_host || !v_host) return fail("ppo_load_adam: null argument");
  if (n != c->L.P) return fail("ppo_load_adam: size mismatch");
  std::vector<float> pm(c->K.size), pv(c->K.size);
  pack_params(c->K, c->L, m_host, pm.data());
  pack_params(c->K, c->L, v_host, pv.data());
  HIP_TRY(hipMemcpyAsync(c->Am, pm.data(), sizeof(float) * c->K.size, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->Av, pv.data(), sizeof(float) * c->K.size, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->adam_step = step;
  return 0;
}

// ------------------------------------------------------------------------------------------
// agent calls
// ------------------------------------------------------------------------------------------
static ActArgs base_act(ppo_t* c) {
  ActArgs a;
  memset(&a, 0, sizeof(a));
  a.P = c->P;
  a.K = c->K;
  a.seed = c->cfg.seed;
  a.rank = c->rank;
  a.store_step = -1;
  a.E = c->cfg.num_envs;
  a.kernel = c->plan.act_kernel;
  a.WSW[0] = c->WSW[0];
  a.WSW[1] = c->WSW[1];
  return a;
}

extern "C" int ppo_get_action_and_value(ppo_t* c, int n, const float* x, int sample_type, const float* action_in,
                                        long env_base, long step_id, float* action, float* logprob, float* entropy,
                                        float* value, void* stream) {
  if (!c || !x) return fail("ppo_get_action_and_value: null argument");
  if (n <= 0) return 0;
  if (sample_type == PPO_GIVEN && !action_in) return fail("ppo_get_action_and_value: GIVEN needs action_in");
  if (sample_type < 0 || sample_type > PPO_ROACH || (sample_type == PPO_ROACH && c->K.kind != PPO_NET_LN_BETA))
    return fail("Unsupported sample type used. Sample type: " + std::to_string(sample_type));
  ActArgs a = base_act(c);
  a.n = n;
  a.x = x;
  a.ldx = c->K.O;
  a.mode = sample_type;
  a.need_actor = (action || logprob || entropy) ? 1 : 0;
  a.action_in = action_in;
  a.env_base = env_base;
  a.step_id = step_id;
  a.action_out = action;
  a.logprob_out = logprob;
  a.entropy_out = entropy;
  a.value_out = value;
  hipStream_t s = S(c, stream);
  ProfScope ps(c, PK_ACT, s);
  if (launch_act(a, s) != 0) return fail("no act kernel for this configuration");
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int ppo_get_value(ppo_t* c, int n, const float* x, float* value, void* stream) {
  return ppo_get_action_and_value(c, n, x, PPO_MEAN, nullptr, 0, 0, nullptr, nullptr, nullptr, value, stream);
}

extern "C" int ppo_rollout_act(ppo_t* c, int step, int e0, int e1, const float* next_obs, const float* next_done,
                               float* action_out, void* stream) {
  if (!c || !next_obs) return fail("ppo_rollout_act: null argument");
  if (step < 0 || step >= c->cfg.num_steps || e0 < 0 || e1 > c->cfg.num_envs || e0 >= e1)
    return fail("ppo_rollout_act: step / env range out of bounds");
  ActArgs a = base_act(c);
  a.n = e1 - e0;
  a.x = next_obs;
  a.ldx = c->K.O;
  a.mode = PPO_SAMPLE;
  a.need_actor = 1;
  a.env_base = e0;
  a.step_id = c->iteration * (long)c->cfg.num_steps + step;
  a.action_out = action_out;
  a.store_step = step;
  a.next_done = next_done;
  a.s_obs = c->buf[PPO_BUF_OBS];
  a.s_actions = c->buf[PPO_BUF_ACTIONS];
  a.s_logp = c->buf[PPO_BUF_LOGPROBS];
  a.s_dones = c->buf[PPO_BUF_DONES];
  a.s_values = c->buf[PPO_BUF_VALUES];
  // values_bx: the critic runs later, once over the stored rows (flush_values: ppo_compute_gae,
  // ppo_rollout_values), with the persistent rollout's kernel, so both collection paths store the
  // same values bit for bit
  a.skip_critic = c->plan.values_bx;
  hipStream_t s = S(c, stream);
  ProfScope ps(c, PK_ACT, s);
  if (launch_act(a, s) != 0) return fail("no act kernel for this configuration");
  if (c->plan.values_bx) {  // groups act concurrently from host threads: an atomic maximum
    int cur = c->values_pending.load();
    while (cur < step + 1 && !c->values_pending.compare_exchange_weak(cur, step + 1)) {
    }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int ppo_rollout_reward(ppo_t* c, int step, int e0, int e1, const float* reward, void* stream) {
  if (!c || !reward) return fail("ppo_rollout_reward: null argument");
  if (step < 0 || step >= c->cfg.num_steps || e0 < 0 || e1 > c->cfg.num_envs || e0 >= e1)
    return fail("ppo_rollout_reward: step / env range out of bounds");
  HIP_TRY(hipMemcpyAsync(c->buf[PPO_BUF_REWARDS] + (size_t)step * c->cfg.num_envs + e0, reward,
                         sizeof(float) * (e1 - e0), hipMemcpyDeviceToDevice, S(c, stream)));
  return 0;
}

static int gae_launch(ppo_t* c, const float* next_value, const float* next_done, int nsteps, hipStream_t s);

// the critic over n contiguous observation rows (k_vbx with the critic's W2 pieces, else launch_values:
// k_values / k_values4, k_values_w at OP = 384 of the AC agent)
int run_values(ppo_t* c, const float* obs, float* values, long n, hipStream_t s) {
  ValuesArgs v;
  v.P = c->P;
  v.K = c->K;
  v.WSW = c->WSW[0];
  v.obs = obs;
  v.values = values;
  v.n = n;
  v.WBX = c->plan.values_bx ? c->WSW[0] + sw_size(c->K.H, c->K.OP) : nullptr;
  ProfScope ps(c, PK_VALUES, s);
  if (v.WBX) return launch_vbx(v, s) == 0 ? 0 : -1;
  return launch_values(v, s);
}
extern "C" int ppo_values(ppo_t* c, long n, const float* obs, float* values, void* stream) {
  if (!c || !obs || !values) return fail("ppo_values: null argument");
  if (n <= 0) return fail("ppo_values: n must be positive, got " + std::to_string(n));
  // no batched critic kernel for the shape (the AC agent above 8 actions below OP = 384): k_act3's critic
  if (rollout_supported(c->K) != 0 && values_w_supported(c->K) != 0) {
    if (n > 0x7fffffffL) return fail("ppo_values: more than 2^31 - 1 rows at a shape without a batched critic kernel");
    return ppo_get_value(c, (int)n, obs, values, stream);
  }
  if (run_values(c, obs, values, n, S(c, stream)) != 0) return fail("ppo_values: values kernel launch failed");
  HIP_TRY(hipGetLastError());
  return 0;
}
// the deferred critic pass of per-step rollouts (ppo_rollout_act with values_bx): values[t] for every
// step acted so far, over the stored observations
int flush_values(ppo_t* c, hipStream_t s) {
  const int steps = c->values_pending.exchange(0);
  if (steps <= 0) return 0;
  if (run_values(c, c->buf[PPO_BUF_OBS], c->buf[PPO_BUF_VALUES], (long)steps * c->cfg.num_envs, s) != 0)
    return fail("ppo_rollout_values: critic kernel launch failed");
  HIP_TRY(hipGetLastError());
  return 0;
}
extern "C" int ppo_rollout_values(ppo_t* c, void* stream) {
  if (!c) return fail("ppo_rollout_values: null argument");
  return flush_values(c, S(c, stream));
}

extern "C" int ppo_compute_gae(ppo_t* c, const float* next_obs, const float* next_done, int nsteps, void* stream) {
  if (!c || !next_obs || !next_done) return fail("ppo_compute_gae: null argument");
  if (nsteps <= 0 || nsteps > c->cfg.num_steps) return fail("ppo_compute_gae: bad step count");
  hipStream_t s = S(c, stream);
  if (int rc = flush_values(c, s)) return rc;
  if (rollout_supported(c->K) == 0) {
    // the bootstrap value with the critic pass that fills values[t] on the persistent path
    if (run_values(c, next_obs, c->next_value, c->cfg.num_envs, s) != 0)
      return fail("ppo_compute_gae: values kernel launch failed");
  } else {
    int rc = ppo_get_value(c, c->cfg.num_envs, next_obs, c->next_value, s);
    if (rc) return rc;
  }
  return gae_launch(c, c->next_value, next_done, nsteps, s);
}

extern "C" int ppo_gae_from_values(ppo_t* c, const float* next_value, const float* next_done, int nsteps,
                                   void* stream) {
  if (!c || !next_value || !next_done) return fail("ppo_gae_from_values: null argument");
  if (nsteps <= 0 || nsteps > c->cfg.num_steps) return fail("ppo_gae_from_values: bad step count");
  if (int rc = flush_values(c, S(c, stream))) return rc;
  return gae_launch(c, next_value, next_done, nsteps, S(c, stream));
}

static int gae_launch(ppo_t* c, const float* next_value, const float* next_done, int nsteps, hipStream_t s) {
  // a partial collection (DD-PPO preemption, nsteps < num_steps): the reference's recurrence bootstraps
  // the last collected step from the STORED step nsteps (values[t + 1], dones[t + 1] whenever
  // t != num_steps - 1, ac:765-774), which every env executed before it stopped; next_value and
  // next_done are not read then
  if (nsteps < c->cfg.num_steps) {
    next_value = c->buf[PPO_BUF_VALUES] + (size_t)nsteps * c->cfg.num_envs;
    next_done = c->buf[PPO_BUF_DONES] + (size_t)nsteps * c->cfg.num_envs;
  }
  GaeArgs g;
  g.rewards = c->buf[PPO_BUF_REWARDS];
  g.values = c->buf[PPO_BUF_VALUES];
  g.dones = c->buf[PPO_BUF_DONES];
  g.next_value = next_value;
  g.next_done = next_done;
  g.adv = c->buf[PPO_BUF_ADVANTAGES];
  g.ret = c->buf[PPO_BUF_RETURNS];
  g.T = nsteps;
  g.E = c->cfg.num_envs;
  g.gamma = c->cfg.gamma;
  g.lam = c->cfg.gae_lambda;
  ProfScope ps(c, PK_GAE, s);
  launch_gae(g, s, c->plan.gae_scan > 0 || (c->plan.gae_scan < 0 && nsteps >= c->plan.gae_scan_min_t));
  HIP_TRY(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// snapshots / sync
// ------------------------------------------------------------------------------------------
extern "C" int ppo_snapshot_state(ppo_t* c) {
  if (!c) return fail("null ctx");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = c->K.size;
  if (!c->snap) {
    HIP_TRY(hipMalloc(&c->snap, 3 * n * sizeof(float)));
    HIP_TRY(hipEventCreateWithFlags(&c->snap_ev, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&c->snap_stream, hipStreamNonBlocking));
  }
  HIP_TRY(hipMemcpyAsync(c->snap, c->P, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->snap + n, c->Am, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->snap + 2 * n, c->Av, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipEventRecord(c->snap_ev, c->stream));
  c->snap_step = c->adam_step;
  return 0;
}

extern "C" int ppo_read_snapshot(ppo_t* c, float* p, float* m, float* v, long n, long* step) {
  if (!c) return fail("null ctx");
  if (!c->snap) return fail("ppo_read_snapshot: no snapshot taken");
  if (n != c->L.P) return fail("ppo_read_snapshot: size mismatch");
  HIP_TRY(hipSetDevice(c->device));
  const size_t K = c->K.size;
  std::vector<float> h(3 * K);
  // a host wait, not hipStreamWaitEvent: a cross-stream dependency on the context stream is refused
  // while the owner thread captures that stream into the update hipGraph (update_graph=1)
  HIP_TRY(hipEventSynchronize(c->snap_ev));
  HIP_TRY(hipMemcpyAsync(h.data(), c->snap, 3 * K * sizeof(float), hipMemcpyDeviceToHost, c->snap_stream));
  HIP_TRY(hipStreamSynchronize(c->snap_stream));
  if (p) unpack_params(c->K, c->L, h.data(), p);
  if (m) unpack_params(c->K, c->L, h.data() + K, m);
  if (v) unpack_params(c->K, c->L, h.data() + 2 * K, v);
  if (step) *step = c->snap_step;
  return 0;
}

extern "C" int ppo_sync(ppo_t* c) {
  if (!c) return fail("null ctx");
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------
extern "C" int ppo_get_device(const ppo_t* c, int* device, char* pci_bus_id, int len) {
  if (!c || !device) return fail("ppo_get_device: null argument");
  *device = c->device;
  if (pci_bus_id && len > 0) HIP_TRY(hipDeviceGetPCIBusId(pci_bus_id, len, c->device));
  return 0;
}

extern "C" int ppo_kernel_info(const ppo_t* c, char* buf, int len) {
  if (!c || !buf || len <= 0) return fail("ppo_kernel_info: null argument");
  const KernelPlan& kp = c->plan;
  const std::string s = "update=" + kp.upd_name + " dw=" + kp.dw_name + " values=" + kp.values_name + " norm=" + kp.norm_name +
                        (kp.rollout_name.empty() ? "" : " rollout=" + kp.rollout_name);
  snprintf(buf, (size_t)len, "%s", s.c_str());
  return 0;
}

extern "C" int ppo_dw_image_offset(int row, int col) {
  return row < 0 || row >= 16 || col < 0 || col >= 256 || (col & 3) ? -1 : dwso_off(row, col);
}

extern "C" int ppo_set_device(int d) {
  if (int rc = ppo_runtime_check()) return rc;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (d < 0 || d >= ndev)
    return fail("ppo_set_device: device " + std::to_string(d) + " requested but " + std::to_string(ndev) +
                " HIP device(s) are visible");
  HIP_TRY(hipSetDevice(d));
  return 0;
}
extern "C" int ppo_device_count(int* n) { HIP_TRY(hipGetDeviceCount(n)); return 0; }
// The helpers are host-synchronous and device-wide ordered: contexts run on non-blocking streams,
// which are NOT ordered against the legacy null stream that plain hipMemcpy/hipMemset use.
extern "C" int ppo_dev_malloc(void** p, size_t bytes) {
  if (int rc = ppo_runtime_check()) return rc;
  HIP_TRY(hipMalloc(p, bytes ? bytes : 1));
  HIP_TRY(hipMemset(*p, 0, bytes ? bytes : 1));
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}
extern "C" int ppo_dev_free(void* p) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipFree(p));
  return 0;
}
extern "C" int ppo_memcpy_h2d(void* d, const void* h, size_t n) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(d, h, n, hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}
extern "C" int ppo_memcpy_d2h(void* h, const void* d, size_t n) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(h, d, n, hipMemcpyDeviceToHost));
  return 0;
}
extern "C" int ppo_memset_dev(void* d, int v, size_t n) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(d, v, n));
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}
extern "C" int ppo_device_sync(void) { HIP_TRY(hipDeviceSynchronize()); return 0; }

// ------------------------------------------------------------------------------------------
// profiling API
// ------------------------------------------------------------------------------------------
extern "C" int ppo_profile_enable(ppo_t* c, int mask) {
  if (!c) return fail("null ctx");
  c->prof_mask = (unsigned)mask;
  return 0;
}
extern "C" int ppo_profile_read(ppo_t* c, double* ms, long* count, int cap) {
  if (!c) return fail("null ctx");
  prof_drain(c);
  for (int i = 0; i < PK_COUNT && i < cap; ++i) {
    if (ms) ms[i] = c->prof_ms[i];
    if (count) count[i] = c->prof_cnt[i];
  }
  return PK_COUNT;
}
extern "C" const char* ppo_profile_name(int id) { return (id >= 0 && id < PK_COUNT) ? kProfNames[id] : ""; }
extern "C" int ppo_profile_reset(ppo_t* c) {
  if (!c) return fail("null ctx");
  prof_drain(c);
  for (int i = 0; i < PK_COUNT; ++i) {
    c->prof_ms[i] = 0;
    c->prof_cnt[i] = 0;
  }
  return 0;
}
