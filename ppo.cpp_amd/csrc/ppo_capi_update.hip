// ppo_capi_update.hip — ppo_update / ppo_update_ex: the PPO update over the rollout storage.
//
// Every kernel argument that is fixed once create returns is built there, once, into the context's
// UpdatePlan (build_update_plan). An update copies it, sets what varies per call (the permutation, the
// attached communicator's world, lr) and runs the minibatch launch sequence (enqueue_minibatches),
// eagerly or as a replay of its captured hipGraph (replay_graph).
#include "ppo_capi_internal.hpp"

void build_update_plan(ppo_t* c) {
  const ppo_hip_config& cfg = c->cfg;
  const KernelPlan& kp = c->plan;
  const int EP = cfg.update_epochs, MB = c->nmb, M = c->M, H = c->K.H, OP = c->K.OP, A = c->K.A;
  const long B = c->B;
  UpdatePlan& p = c->up;
  // ---- advantage statistics of every minibatch ----
  AdvArgs& aa = p.aa;
  aa.perm = nullptr;  // per call
  aa.adv = c->buf[PPO_BUF_ADVANTAGES];
  aa.stats = c->advstats;
  aa.sq = c->advsq;
  aa.part = c->advpart;
  aa.M = M;
  aa.nmb = EP * MB;
  aa.world = 1;  // per call
  // ---- k_upd / k_upd2 / k_upd32 / k_fwdbwd ----
  UpdArgs& u = p.u;
  memset(&u, 0, sizeof(u));
  u.P = c->P;
  u.W2T[0] = c->W2T[0];
  u.W2T[1] = c->W2T[1];
  u.WSW[0] = c->WSW[0];
  u.WSW[1] = c->WSW[1];
  u.bx = kp.upd_bx;
  u.K = c->K;
  u.sg[0] = c->sg[0];
  u.sg[1] = c->sg[1];
  u.M = M;
  u.tiles_per_block = kp.tiles_per_block;
  u.wlds_off = kp.wlds_off;
  u.obs = c->buf[PPO_BUF_OBS];
  u.actions = c->buf[PPO_BUF_ACTIONS];
  u.logp = c->buf[PPO_BUF_LOGPROBS];
  u.adv = c->buf[PPO_BUF_ADVANTAGES];
  u.ret = c->buf[PPO_BUF_RETURNS];
  u.val = c->buf[PPO_BUF_VALUES];
  u.rows_n = B;
  u.obs_n = B * c->K.O;
  u.clip_coef = cfg.clip_coef;
  u.ent_coef = cfg.ent_coef;
  u.vf_coef = cfg.vf_coef;
  u.inv_m = 1.0f / (float)M;
  u.clip_vloss = cfg.clip_vloss;
  u.norm_adv = cfg.norm_adv;
  u.Xn = c->Xn;
  u.Z1 = c->Z1;
  u.actn_off = kp.upd.actn_off;
  u.acc_off = kp.upd.acc_off;
  u.spar_off = kp.upd.spar_off;
  u.hw_global = kp.upd.hw_global;
  u.trunk_mask = kp.upd_trunk_mask;
  u.sched = kp.upd_sched;
  u.h1_skip = kp.h1_recomp;
  u.hot = kp.upd_hot;
  p.nblk = kp.use_upd ? kp.upd_nblk : kp.nblk;  // workgroups that wrote a slab row (per launch)
  p.nsrow = kp.msplit * p.nblk;                  // slab rows of one minibatch (msplit launches)
  const int nsrow = p.nsrow;
  for (int k = 0; k < 2; ++k) {
    u.H1[k] = c->H1[k];
    u.LNS[k] = c->LNS[k];
    u.DZ1[k] = c->DZ1[k];
    u.DZ2[k] = c->DZ2[k];
    u.slab[k] = c->slab[k];
  }
  // ---- dW ----
  DwArgs& dw = p.dw;
  memset(&dw, 0, sizeof(dw));
  dw.M = M;
  dw.rows_per_chunk = kp.rows_per_chunk;
  dw.slices = kp.dw_slices;
  dw.fused = kp.dw_fused;
  dw.dma = kp.dw_dma;
  dw.bx = kp.dw_dma ? kp.dw_bx : 0;
  dw.h1_recompute = kp.h1_recomp;
  dw.split_once = kp.dw_so;
  dw.kl1 = (c->K.O == 16 * (c->K.OP / 16 - 1) + 1) ? 1 : 4;
  dw.xn = c->Xn;
  dw.obs = c->buf[PPO_BUF_OBS];
  dw.O = c->K.O;
  dw.obs_n = B * c->K.O;
  dw.slab_stride = (long)H * H + (long)H * OP;
  for (int k = 0; k < 2; ++k) {
    dw.dz2[k] = c->DZ2[k];
    dw.h1[k] = c->H1[k];
    dw.lns[k] = c->LNS[k];
    dw.w1sw[k] = c->WSW[k];
    dw.b1[k] = c->P + c->K.tr[k].b1;
    dw.g1[k] = c->P + c->K.tr[k].g1;
    dw.be1[k] = c->P + c->K.tr[k].be1;
    dw.dz1[k] = c->DZ1[k];
    dw.slab[k] = c->dwslab[k];
  }
  // ---- slab -> packed gradient segments ----
  ColsumArgs& cs = p.cs;
  memset(&cs, 0, sizeof(cs));
  int ns = 0;
  long maxlen = 0;
  auto seg = [&](const float* src, long stride, int count, int len, float* dst, float scale) {
    cs.seg[ns++] = ColsumSeg{src, dst, stride, count, len, scale};
    maxlen = std::max(maxlen, (long)len);
  };
  const bool ln = cfg.net_kind == PPO_NET_LN_BETA;
  for (int k = 0; k < 2; ++k) {
    const TrunkDev& T = c->K.tr[k];
    seg(c->dwslab[k], dw.slab_stride, kp.msplit * kp.nchunks, H * H, c->G + T.W2, 1.f);
    seg(c->dwslab[k] + (long)H * H, dw.slab_stride, kp.msplit * kp.nchunks, H * OP, c->G + T.W1, 1.f);
    const SmallGradLayout& g = c->sg[k];
    const float* sl = c->slab[k];
    seg(sl + g.b1, g.size, nsrow, H, c->G + T.b1, 1.f);
    seg(sl + g.b2, g.size, nsrow, H, c->G + T.b2, 1.f);
    if (ln) {
      seg(sl + g.g1, g.size, nsrow, H, c->G + T.g1, 1.f);
      seg(sl + g.be1, g.size, nsrow, H, c->G + T.be1, 1.f);
      seg(sl + g.g2, g.size, nsrow, H, c->G + T.g2, 1.f);
      seg(sl + g.be2, g.size, nsrow, H, c->G + T.be2, 1.f);
    }
    if (k == 0) {
      seg(sl + g.hW, g.size, nsrow, H, c->G + c->K.cW3, 1.f);
      seg(sl + g.hb, g.size, nsrow, 1, c->G + c->K.cb3, 1.f);
    } else if (!ln) {
      seg(sl + g.hW, g.size, nsrow, A * H, c->G + c->K.aW3, 1.f);
      seg(sl + g.hb, g.size, nsrow, A, c->G + c->K.ab3, 1.f);
      seg(sl + g.ls, g.size, nsrow, A, c->G + c->K.logstd, 1.f);
    } else {
      seg(sl + g.hW, g.size, nsrow, A * H, c->G + c->K.aW3, 1.f);
      seg(sl + g.hW + A * H, g.size, nsrow, A * H, c->G + c->K.bW3, 1.f);
      seg(sl + g.hb, g.size, nsrow, A, c->G + c->K.ab3, 1.f);
      seg(sl + g.hb + A, g.size, nsrow, A, c->G + c->K.bb3, 1.f);
    }
  }
  const int stats_seg0 = ns;  // the three statistics segments: their sources are fixed, their destination is
  ns += 3;                    // the minibatch's row of mbstats (enqueue_minibatches)
  p.ns = ns;
  p.maxlen = maxlen;
  p.stats_seg0 = stats_seg0;
  // ---- clip_grad_norm_ + Adam ----
  NormArgs& na = p.na;
  memset(&na, 0, sizeof(na));
  na.grad = c->G;
  na.max_norm = cfg.max_grad_norm;
  na.out = c->normout;
  na.part = c->gnpart;
  for (int t = 0; t < c->K.nt; ++t)
    if (c->K.grad[t]) {
      na.off[na.nt] = c->K.poff[t];
      na.len[na.nt] = c->K.rows[t] * c->K.ld[t];
      na.nt++;
    }
  // gradnorm=fold: every norm tensor must be exactly one gradient segment of the column sums (and no
  // all-reduce may change the gradient between them and the norm: ppo_update_ex); otherwise k_gradnorm runs
  bool fold = kp.gn_fold && !kp.gradstep;
  if (fold) {
    int hits[PPO_LAYOUT_MAX_TENSORS] = {};
    for (int k = 0; k < stats_seg0; ++k) {
      cs.seg_t[k] = -1;
      const long off = (long)(cs.seg[k].dst - c->G);
      for (int t = 0; t < na.nt; ++t)
        if (na.off[t] == off && na.len[t] == cs.seg[k].len) { cs.seg_t[k] = t; hits[t]++; }
    }
    for (int t = 0; t < na.nt; ++t) fold = fold && hits[t] == 1;
    long tiles = 0;
    for (int k = 0; k < stats_seg0 + 3; ++k) tiles += (k < stats_seg0 ? (cs.seg[k].len + 63) / 64 : 1);
    fold = fold && tiles <= (long)c->K.size / 64 + 2 * PPO_MAX_SEGS + 64;
  }
  for (int k = stats_seg0; k < stats_seg0 + 3; ++k) cs.seg_t[k] = -1;
  p.fold_ok = fold;
  cs.fold = 0;  // per call
  cs.sq = c->cs_sq;
  cs.cnt = c->cs_cnt;
  cs.part = c->gnpart;
  int tb = -1;
  for (int t = 0; t < c->K.nt; ++t)
    if (c->K.grad[t]) { tb = c->K.poff[t]; break; }
  AdamArgs& ad = p.ad;
  memset(&ad, 0, sizeof(ad));
  ad.param = c->P;
  ad.grad = c->G;
  ad.m = c->Am;
  ad.v = c->Av;
  ad.begin = tb;
  ad.n = c->K.size - tb;
  ad.norm_out = c->normout;
  ad.part = c->gnpart;
  ad.nt = na.nt;
  ad.max_norm = cfg.max_grad_norm;
  ad.eps = cfg.adam_eps;
  ad.H = H;
  ad.OP = c->K.OP;
  for (int k = 0; k < 2; ++k) {
    ad.w2_off[k] = c->K.tr[k].W2;
    ad.w2t[k] = c->W2T[k];
    ad.w1_off[k] = c->K.tr[k].W1;
    ad.wsw[k] = c->WSW[k];
  }
  ad.bx = kp.upd_bx;
  p.tb = tb;
  p.trainable_n = c->K.size - tb;
}

// The minibatch launch sequence of one update: EP epochs x MB minibatches of
// {k_l1g} msplit x {k_upd, dW} k_colsum {all-reduce} {k_gradnorm} k_adam.
//
// What the update graph relies on: every kernel argument enqueued here is identical from call to call,
// except through the two things that are handed in and change, the permutation buffer (a replay is
// re-captured when it moves) and, with graph, the Adam step constants, which the kernels read from
// c->sched[gi] (refilled by the host before each replay). Everything else comes from p, which is the
// context's UpdatePlan: built once at create, never from per-call state. lr is read on the eager path only.
static int enqueue_minibatches(ppo_t* c, UpdatePlan& p, const int32_t* perms, float lr, bool multi, bool graph) {
  const KernelPlan& kp = c->plan;
  const int EP = c->cfg.update_epochs, MB = c->nmb, M = c->M, H = c->K.H, OP = c->K.OP;
  const long B = c->B;
  hipStream_t s = c->stream;
  UpdArgs& u = p.u;
  DwArgs& dw = p.dw;
  ColsumArgs& cs = p.cs;
  AdamArgs& ad = p.ad;
  const int nblk = p.nblk, nsrow = p.nsrow, stats_seg0 = p.stats_seg0;
  for (int e = 0; e < EP; ++e) {
    for (int mb = 0; mb < MB; ++mb) {
      const int gi = e * MB + mb;
      u.perm = perms + (size_t)e * B + (size_t)mb * M;
      u.adv_stats = c->advstats + 2 * gi;
      if (kp.use_upd2) dw.perm = u.perm;  // k_dw gathers dW1's input rows itself
      if (kp.upd2_split) {
        ProfScope ps(c, PK_L1G, s);
        if (launch_l1g(u, s) != 0) return fail("k_l1g: unsupported configuration");
      }
      // msplit > 1: launch pairs over consecutive Mq-row ranges of the minibatch's permutation; each pair's
      // hand-off rows start at row 0 of the hand-off buffers (reused while cache-resident), its slab rows
      // and dW partial rows follow the previous pair's (the column sums add them all, in pair order);
      // the loss scale stays 1 / M of the whole minibatch
      for (int q = 0; q < kp.msplit; ++q) {
        const int mq = std::min(kp.Mq, M - q * kp.Mq);
        UpdArgs uq = u;
        DwArgs dq = dw;
        if (kp.msplit > 1) {
          uq.perm = u.perm + (size_t)q * kp.Mq;
          uq.M = mq;
          dq.M = mq;
          for (int k = 0; k < 2; ++k) {
            uq.slab[k] = c->slab[k] + (size_t)q * nblk * c->sg[k].size;
            dq.slab[k] = c->dwslab[k] + (size_t)q * kp.nchunks * dw.slab_stride;
          }
        }
        {
          ProfScope ps(c, PK_FWDBWD, s);
          const int rc_ = kp.use_upd2  ? launch_upd2(uq, kp.upd_nblk, kp.upd.lds_bytes, s, kp.upd2_split)
                          : kp.use_upd32 ? launch_upd32(uq, c->sg[1].nh, kp.upd_nblk, kp.upd.lds_bytes, s, kp.upd32_mix)
                          : kp.use_upd ? launch_upd(uq, c->sg[1].nh, kp.upd_nblk, kp.upd.lds_bytes, s)
                                       : launch_fwdbwd(uq, nblk, kp.lds_bytes, s);
          if (rc_ != 0) return fail("no update kernel for this configuration");
        }
        {
          ProfScope ps(c, PK_DW2, s);
          const int nch = (mq + kp.rows_per_chunk - 1) / kp.rows_per_chunk;
          const int rc_ = kp.use_upd2 ? launch_dw2(dq, OP, kp.nchunks, s) : launch_dw(dq, H, OP, nch, s);
          if (rc_ != 0) return fail("no dW kernel for this configuration");
          if (nch < kp.nchunks && !kp.use_upd2)  // a shorter last pair: its unused partial rows must add 0
            for (int k = 0; k < 2; ++k)
              HIP_TRY(hipMemsetAsync(dq.slab[k] + (size_t)nch * dw.slab_stride, 0,
                                     sizeof(float) * (size_t)(kp.nchunks - nch) * dw.slab_stride, s));
        }
      }
      float* st = c->mbstats + 8 * gi;
      cs.seg[stats_seg0 + 0] = ColsumSeg{c->slab[1] + c->sg[1].stats + ST_PG, st + ST_PG, c->sg[1].size, nsrow, 1, 1.f / M};
      cs.seg[stats_seg0 + 1] = ColsumSeg{c->slab[0] + c->sg[0].stats + ST_V, st + ST_V, c->sg[0].size, nsrow, 1, 0.5f / M};
      cs.seg[stats_seg0 + 2] = ColsumSeg{c->slab[1] + c->sg[1].stats + ST_ENT, st + ST_ENT, c->sg[1].size, nsrow, 4, 1.f / M};
      {
        ProfScope ps(c, PK_COLSUM, s);
        launch_colsum(cs, p.ns, p.maxlen, s);
      }
      if (multi && allreduce(c, c->G + p.tb, p.trainable_n, 1, s)) return -3;  // ac:877-885, before the clip
      if (graph) {
        ad.sched = c->sched;
        ad.gi = gi;
      } else {
        c->adam_step += 1;
        const double bc1 = 1.0 - std::pow(0.9, (double)c->adam_step);
        const double bc2 = 1.0 - std::pow(0.999, (double)c->adam_step);
        ad.step_size = (float)((double)lr / bc1);
        ad.sbc2 = (float)std::sqrt(bc2);
      }
      ad.stat_out = st + 6;  // the total norm of this minibatch next to its loss stats
      if (kp.gradstep) {  // clip_grad_norm_ + Adam: one cooperative launch (profile class "adam")
        ProfScope ps(c, PK_ADAM, s);
        if (launch_gradstep(p.na, ad, c->gs_bar, &c->gs_count, s) != 0) return fail("k_gradstep launch failed");
      } else {
        if (!cs.fold) {
          ProfScope ps(c, PK_GRADNORM, s);
          launch_gradnorm(p.na, s);
        }
        ProfScope ps(c, PK_ADAM, s);
        launch_adam(ad, s);
      }
    }
  }
  return 0;
}

// One update as a replay of the captured launch sequence (update_graph, one process, split clip + Adam,
// no profiling events): captured on the first call that comes here, which is the context's second update
// (the first, eager, warms the launchers' one-time attribute calls), and re-captured when the
// permutation buffer changes. Before each replay the host writes the Adam step constants of its
// minibatches into c->sched.
static int replay_graph(ppo_t* c, UpdatePlan& p, const int32_t* perms, float lr) {
  hipStream_t s = c->stream;
  const int n = c->cfg.update_epochs * c->nmb;
  if (!c->sched) {
    if (dmalloc(&c->sched, 2 * (size_t)n)) return -2;
    for (int i = 0; i < 2; ++i) {
      HIP_TRY(hipHostMalloc((void**)&c->sched_host[i], sizeof(float) * 2 * n, hipHostMallocDefault));
      HIP_TRY(hipEventCreateWithFlags(&c->sched_ev[i], hipEventDisableTiming));
    }
  }
  // the staging buffer alternates per replay; before refilling one, wait until the copy that last
  // read it (two replays ago) has completed — back-to-back replays never overwrite a pending copy
  float* sh = c->sched_host[c->sched_flip];
  HIP_TRY(hipEventSynchronize(c->sched_ev[c->sched_flip]));
  for (int gi = 0; gi < n; ++gi) {  // the eager path's per-step constants, same expressions
    const long t = c->adam_step + 1 + gi;
    const double bc1 = 1.0 - std::pow(0.9, (double)t);
    const double bc2 = 1.0 - std::pow(0.999, (double)t);
    sh[2 * gi] = (float)((double)lr / bc1);
    sh[2 * gi + 1] = (float)std::sqrt(bc2);
  }
  HIP_TRY(hipMemcpyAsync(c->sched, sh, sizeof(float) * 2 * n, hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(c->sched_ev[c->sched_flip], s));
  c->sched_flip ^= 1;
  if (!c->upd_exec || c->upd_exec_perms != perms) {
    if (c->upd_exec) (void)hipGraphExecDestroy(c->upd_exec);
    c->upd_exec = nullptr;
    HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_minibatches(c, p, perms, lr, false, true);
    hipGraph_t g = nullptr;
    const hipError_t ec = hipStreamEndCapture(s, &g);
    if (rc != 0) {
      if (g) (void)hipGraphDestroy(g);
      return rc;
    }
    if (ec != hipSuccess) return fail(std::string("ppo_update: graph capture: ") + hipGetErrorString(ec));
    const hipError_t ei = hipGraphInstantiate(&c->upd_exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) {
      c->upd_exec = nullptr;
      return fail(std::string("ppo_update: graph instantiate: ") + hipGetErrorString(ei));
    }
    c->upd_exec_perms = perms;
  }
  HIP_TRY(hipGraphLaunch(c->upd_exec, s));
  c->adam_step += n;
  return 0;
}

// Permutations of one update (torch::randperm per epoch, ppo:490 / ac:804) into c->perms.
// A partial collection of nsteps < num_steps (DD-PPO preemption, ac:803-810): the permutation runs
// over the Bc = nsteps * E collected samples (the first nsteps rows of the [T, E] storage) and is
// repeated and truncated to the per-device batch, b_inds.repeat(ceil(B / Bc))[:B]
static int fill_perms(ppo_t* c, int nsteps, hipStream_t s) {
  ProfScope ps(c, PK_PERM, s);
  const int EP = c->cfg.update_epochs;
  const long B = c->B, Bc = (long)nsteps * c->cfg.num_envs;
  for (int e = 0; e < EP; ++e) {
    int32_t* dst = c->perms + (size_t)e * B;
    launch_perm(dst, (uint32_t)Bc, make_perm_key(c->cfg.seed, c->rank, c->iteration * (long)EP + e, Bc), s);
    for (long have = Bc; have < B;) {  // doubling copies of the periodic prefix
      const long n = std::min(have, B - have);
      HIP_TRY(hipMemcpyAsync(dst + have, dst, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, s));
      have += n;
    }
  }
  return 0;
}

extern "C" int ppo_update(ppo_t* c, float lr, const int32_t* perms_dev, ppo_update_stats* out) {
  if (!c) return fail("ppo_update: null ctx");
  return ppo_update_ex(c, lr, c->cfg.num_steps, perms_dev, out);
}

extern "C" int ppo_update_ex(ppo_t* c, float lr, int nsteps, const int32_t* perms_dev, ppo_update_stats* out) {
  if (!c) return fail("ppo_update: null ctx");
  if (c->plan.no_update) return fail("ppo_update: the context was created with update=off");
  if (nsteps <= 0 || nsteps > c->cfg.num_steps) return fail("ppo_update: bad collected step count");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const ppo_hip_config& cfg = c->cfg;
  const KernelPlan& kp = c->plan;
  const int EP = cfg.update_epochs, MB = c->nmb;
  const bool multi = distributed(c);
  if (cfg.world_size > 1 && !multi)
    return fail("ppo_update: world_size " + std::to_string(cfg.world_size) +
                " but no communicator attached (ppo_comm_init / ppo_comm_init_host)");
  if (int rc = flush_values(c, s)) return rc;  // old values of a per-step rollout whose GAE came from elsewhere
  const int32_t* perms = perms_dev;
  if (!perms) {
    if (int rc = fill_perms(c, nsteps, s)) return rc;
    perms = c->perms;
  }
  // the create-time arguments, and what a communicator attached or detached since create changes
  UpdatePlan p = c->up;
  p.aa.perm = perms;
  p.aa.world = multi ? c->world : 1;
  p.cs.fold = p.fold_ok && !multi ? 1 : 0;
  // ---- advantage statistics of every minibatch (ppo:511; distributed ac:833-846) ----
  if (cfg.norm_adv) {
    ProfScope ps(c, PK_ADV, s);
    launch_adv_sum(p.aa, s);
    if (multi && allreduce(c, c->advstats, 2L * EP * MB, 1, s)) return -3;
    launch_adv_sq(p.aa, multi ? 0 : 1, s);
    if (multi) {
      if (allreduce(c, c->advsq, (long)EP * MB, 0, s)) return -3;
      launch_adv_finalize(p.aa, s);
    }
  }
  // ---- the minibatches ----
  // auto stays eager for a caller that takes snapshots (the CLIs' checkpoint writer thread reads them
  // while the next update runs: a capture then failed on the GPU box, "operation failed due to a previous
  // error during capture"); update_graph=1 keeps the graph with snapshots (single-threaded callers)
  const bool use_graph = kp.update_graph && !multi && !kp.gradstep && c->prof_mask == 0 && !(kp.update_graph_auto && c->snap);
  if (int rc = use_graph && c->upd_calls > 0 ? replay_graph(c, p, perms, lr) : enqueue_minibatches(c, p, perms, lr, multi, false))
    return rc;
  c->upd_calls += 1;
  HIP_TRY(hipGetLastError());
  c->iteration += 1;
  if (out) {
    std::vector<float> h((size_t)8 * EP * MB);
    if (multi && allreduce(c, c->mbstats, 8L * EP * MB, 1, s)) return -3;  // logging averages, ac:895-901
    HIP_TRY(hipMemcpyAsync(h.data(), c->mbstats, sizeof(float) * h.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const float* last = h.data() + 8 * (EP * MB - 1);
    out->pg_loss = last[ST_PG];
    out->v_loss = last[ST_V];
    out->entropy = last[ST_ENT];
    out->old_approx_kl = last[ST_OKL];
    out->approx_kl = last[ST_KL];
    double cf = 0;
    for (int i = 0; i < EP * MB; ++i) cf += h[8 * i + ST_CF];
    out->clipfrac = (float)(cf / (EP * MB));
    out->grad_norm = last[6];
    out->minibatches = EP * MB;
  }
  return 0;
}

extern "C" int ppo_debug_last_grad(ppo_t* c, float* host, long n) {
  if (!c || !host) return fail("ppo_debug_last_grad: null argument");
  if (n != c->L.P) return fail("ppo_debug_last_grad: size mismatch");
  std::vector<float> packed(c->K.size);
  HIP_TRY(hipMemcpyAsync(packed.data(), c->G, sizeof(float) * c->K.size, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  unpack_params(c->K, c->L, packed.data(), host);
  return 0;
}
