// ppo_capi_plan.hip — which kernels a context runs: the parser of ppo_create_ex's options, what each
// option's auto stands for (with the measurement that settled it), and plan_kernels, which turns the
// config and the options into the KernelPlan (ppo_capi_internal.hpp) or refuses.
//
// plan_kernels runs before anything is allocated: every refusal of a configuration comes from here, in a
// fixed order, and ppo_create_ex sizes its allocations from the finished plan (the slabs from msplit,
// nblk and upd_nblk; the dW partial rows from msplit x nchunks; LNS under h1_recomp; Z1 under
// upd2_split). The only HIP calls are the *_supported functions' LDS attribute calls.
#include "ppo_capi_internal.hpp"

// auto = the single k_upd2: the split form measured slower on cfg2 (round 4, profiles/r04/cfg2_split/:
// 101.3 vs 92.9 ms per iteration; k_l1g 66 us = 0.61 of peak per launch, the tail 94 us at 3 per CU)
static constexpr int kUpd2SplitAuto = 0;
// dw_mfma=auto: the fused dW as six exact bf16 piece products (k_dwf_bx, bf16x6: k_upd's six; the
// dropped mid.lo + lo.mid + lo.lo are < 2^-21 of each product). With k_upd on its split-bf16 form the
// metric iteration runs 17.32 (fp32 MFMA dW) -> 16.65 (bf16x9) ms, and bf16x9 17.02 -> bf16x6 16.55 ms
// on another box (profiles/r05/bx6/); against the fp64 oracle every dW tensor stays within 1.5x of the
// fp32 MFMA's error (test_split_bf16_dw_is_as_accurate_as_fp32_mfma)
static constexpr int kDwBxAuto = 6;
// upd_mfma=auto: k_upd's split-bf16 form (bx6) wherever it is instantiated (LayerNorm-Beta agent,
// H = 256, one head tile): as exact as the fp32 MFMA form against the oracle
// (test_upd_bx6_is_as_accurate_as_fp32_mfma), k_upd 0.775 -> 0.606 ms per launch at the metric config
static constexpr int kUpdBxAuto = 1;
// upd_mfma=auto for the 64-wide agent: k_upd2's layer 1 as split-bf16 piece products where instantiated
static constexpr int kUpd2BxAuto = 1;
// gae=auto: k_gae_scan from this many steps on (cfg1 / cfg2's T = 2 048: 16 segments per env; within
// 1e-5 of the serial recurrence and of the golden vectors, test_gae_scan_vs_golden), the bit-exact serial
// k_gae below it (the metric's T = 128: 13 us, < 0.1 % of the iteration). cfg2: 0.186 -> 0.107 ms
// (profiles/r05/gae_scan/)
static constexpr int kGaeScanMinT = 512;
// upd_split=auto: launch pairs per minibatch (see KernelPlan::msplit); 1 until measured
static int kUpdSplitAuto(int M) { (void)M; return 1; }
// h1_handoff=auto: H1 stored. Recomputing it in k_dwf_bx (bitwise the same, test_h1_recompute_is_bitwise_the_
// stored_h1) took k_upd 0.605 -> 0.573 ms per launch but k_dwf_bx 217 -> 255 us (its extra fp32 MFMAs and a
// barrier per stage): 15.97 -> 16.04 ms per metric iteration (profiles/r06/h1_recompute/)
static constexpr bool kH1RecomputeAuto = false;
// dw_stage=auto: the split-once form (k_dwf_so, bitwise k_dwf_bx's dW: test_gpu_dw_split_once) wherever it
// applies. Against the parent's k_dwf_bx on the same box, interleaved runs: dW 3.46 -> 2.98 ms per metric
// iteration (216 -> 186 us per launch), the iteration 15.62-15.80 -> 15.17-15.28 ms (2-3.7 % on four boxes,
// every run of it faster than every run of k_dwf_bx on its box); the E = 512 shard unchanged, 3.40-3.41 ->
// 3.39-3.41 ms (profiles/r07/dw_split_once/)
static constexpr bool kDwSplitOnceAuto = true;
// update_graph=auto: the graph for minibatches of at most this many rows, where launch overhead shows
// (cfg1's 64 rows: 17.9 -> 17.4 ms per iteration); at cfg2 / cfg4 / the shards / the metric config it
// measured equal or 0.5-1 % slower (profiles/r06/update_graph/)
static constexpr int kUpdGraphAutoRows = 4096;
// gradnorm=auto: k_gradnorm. The fold measured slower everywhere (E = 512 shard 3.44 -> 3.78 ms, cfg2 87.5 -> 88.7,
// cfg1 17.4 -> 17.9: each tile's write-through store + counter round trip costs more than the launch it
// saves; profiles/r06/gradnorm_fold/)
static constexpr int kGradnormFoldAuto = 0;

int parse_create_options(const char* opts, CreateOptions* o) {
  if (!opts) return 0;
  std::string s(opts);
  size_t pos = 0;
  while (pos < s.size()) {
    size_t end = s.find(',', pos);
    if (end == std::string::npos) end = s.size();
    const std::string kv = s.substr(pos, end - pos);
    pos = end + 1;
    if (kv.empty()) continue;
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) return fail("ppo_create_ex: option without '=': " + kv);
    const std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
    if (k == "upd_kernel" && (v == "auto" || v == "fwdbwd")) o->upd_kernel = v == "fwdbwd";
    else if (k == "update" && (v == "on" || v == "off")) o->update = v == "on";
    else if (k == "act_kernel" && (v == "auto" || v == "2" || v == "4")) o->act_kernel = v == "auto" ? 0 : v[0] - '0';
    else if (k == "dw_fused" && (v == "0" || v == "1")) o->dw_fused = v[0] - '0';
    else if (k == "rollout" && (v == "auto" || v == "per_step"))
      o->rollout = v == "auto" ? PPO_ROLLOUT_AUTO : PPO_ROLLOUT_PER_STEP;
    else if (k == "gradstep" && (v == "fused" || v == "split")) o->gradstep = v == "fused";
    else if (k == "gradnorm" && (v == "auto" || v == "slices" || v == "fold")) o->gradnorm = v == "auto" ? -1 : v == "fold";
    else if (k == "dw_rows" && !v.empty() && v.size() <= 5 && v.find_first_not_of("0123456789") == std::string::npos &&
             atoi(v.c_str()) % 16 == 0 && atoi(v.c_str()) >= 16 && atoi(v.c_str()) <= 65536)
      o->dw_rows = atoi(v.c_str());  // at most 5 digits: no overflow, no exception across the C-ABI
    else if (k == "dw_slices" && (v == "1" || v == "2")) o->dw_slices = v[0] - '0';
    else if (k == "dw_dma" && (v == "0" || v == "1")) o->dw_dma = v[0] - '0';
    else if (k == "gae" && (v == "auto" || v == "serial" || v == "scan")) o->gae_scan = v == "auto" ? -1 : v == "scan";
    else if (k == "h1_handoff" && (v == "auto" || v == "store" || v == "recompute"))
      o->h1_handoff = v == "auto" ? -1 : v == "recompute";
    else if (k == "dw_stage" && (v == "auto" || v == "dma" || v == "split_once"))
      o->dw_stage = v == "auto" ? -1 : v == "split_once";
    else if (k == "upd_split" && (v == "auto" || v == "1" || v == "2" || v == "4" || v == "8"))
      o->upd_split = v == "auto" ? 0 : v[0] - '0';
    else if (k == "values_mfma" && (v == "auto" || v == "f32" || v == "bx6"))
      o->values_mfma = v == "auto" ? -1 : v == "f32" ? 0 : 6;
    else if (k == "dw_mfma" && (v == "auto" || v == "f32" || v == "bf16x9" || v == "bf16x8" || v == "bf16x6"))
      o->dw_bx = v == "auto" ? -1 : v == "f32" ? 0 : v == "bf16x9" ? 9 : v == "bf16x8" ? 8 : 6;
    else if (k == "update_graph" && (v == "auto" || v == "0" || v == "1")) o->update_graph = v == "auto" ? -1 : v[0] - '0';
    else if (k == "rollout_kernel" && (v == "auto" || v == "mfma" || v == "valu" || v == "split"))
      o->rollout_kernel = v == "auto" ? 0 : v == "mfma" ? 1 : v == "valu" ? 2 : 3;
    else if (k == "upd2_split" && (v == "auto" || v == "0" || v == "2" || v == "3")) o->upd2_split = v == "auto" ? -1 : v[0] - '0';
    else if (k == "upd_mfma" && (v == "auto" || v == "16" || v == "32" || v == "mix" || v == "bx6"))
      o->upd_mfma = v == "auto" ? 0 : v == "mix" ? 1 : v == "bx6" ? 6 : atoi(v.c_str());
    else return fail("ppo_create_ex: unknown option or value: " + kv);
  }
  return 0;
}

// The names ppo_kernel_info prints, from the finished selection. The dW name is decided here, once: it
// must agree with the dispatch of launch_dw / launch_dw2 (ppo_kernels.hip), which pick the kernel from
// the same DwArgs flags and (H, OP) at every launch.
static void name_kernels(const PackedLayout& K, KernelPlan* p) {
  p->upd_name = p->use_upd2    ? (p->upd2_split ? "k_l1g+k_upd2" : p->upd_bx ? "k_upd2/bx6" : "k_upd2/f32")
                : p->use_upd32 ? (p->upd32_mix ? "k_upd32/mix" : "k_upd32")
                : p->use_upd   ? (p->upd_bx ? "k_upd/bx6" : "k_upd/f32")
                               : "k_fwdbwd";
  if (p->use_upd && !p->use_upd2 && p->upd.hw_global) p->upd_name += "/hwg";  // actor dW3 sums in its slab row
  const int H = K.H, OP = K.OP;
  const bool fused = p->dw_fused && H == 256 && (OP == 16 || OP == 32);
  const std::string bxs = p->dw_bx ? "/bf16x" + std::to_string(p->dw_bx) : "/f32";
  p->dw_name = p->use_upd2 ? (p->dw_dma && OP == 384 && K.O % 4 == 0 ? "k_dw2_dma" + bxs : "k_dw2")
               : fused ? (!p->dw_dma ? "k_dwf" : p->dw_bx ? "k_dwf_bx/bf16x" + std::to_string(p->dw_bx) + (p->h1_recomp ? "/h1rc" : p->dw_so ? "/split_once" : "")
                                                    : "k_dwf_dma/f32")
               : (p->dw_dma && H == 256 && OP == 112) ? "k_dw_dma" + bxs
                                                      : "k_dw";
  p->values_name = values_w_supported(K) == 0 ? "k_values_w/f32" : rollout_supported(K) != 0 ? "k_act" : p->values_bx ? "k_vbx/bx6"
                   : K.kind == PPO_NET_TANH_NORMAL ? "k_values4/f32" : "k_values/f32";
  // the create option, not the per-update decision (a communicator turns the fold off)
  p->norm_name = p->gn_fold && !p->gradstep ? "k_colsum" : p->gradstep ? "k_gradstep" : "k_gradnorm";
  p->rollout_name = p->rollout_kernel == 3 ? "k_rollout_s" : "";  // the opt-in rollout kernel (create and ppo_rollout_synth refuse what would bypass it)
}

int plan_kernels(const ppo_hip_config& cfg, const PackedLayout& K, const SmallGradLayout (&sg)[2], const CreateOptions& opt,
                 KernelPlan* p) {
  const int H = cfg.hidden, A = cfg.act_dim, O = cfg.obs_dim, OP = K.OP, kind = cfg.net_kind;
  const long B = (long)cfg.num_envs * cfg.num_steps;
  const int M = (int)(B / cfg.num_minibatches);
  {
    const int nto = OP / 16;
    bool ok = false;
    const int sup[][3] = {{256, 1, 1}, {256, 1, 2}, {256, 1, 7}, {256, 1, 24}, {64, 0, 1}, {64, 0, 2},
                          {64, 0, 7}, {64, 0, 24}, {64, 1, 2}, {256, 0, 2}};
    for (auto& s3 : sup)
      if (s3[0] == H && s3[1] == kind && s3[2] == nto) ok = true;
    if (!ok) return fail("ppo_create: no kernel instantiation for this (hidden, net_kind, obs_dim)");
  }
  // kernel selection: the options of ppo_create_ex (A/B comparisons of complete, tested kernels);
  // the diagnostic build (PPO_DIAG) also reads the measurement scripts' environment switches
  p->act_kernel = opt.act_kernel;
  p->dw_fused = opt.dw_fused;
  p->dw_dma = opt.dw_dma;
  p->gae_scan = opt.gae_scan;
  p->gae_scan_min_t = kGaeScanMinT;
  p->dw_bx = opt.dw_bx >= 0 ? opt.dw_bx : kDwBxAuto;
  p->gradstep = opt.gradstep;
  p->gn_fold = opt.gradnorm >= 0 ? opt.gradnorm : kGradnormFoldAuto;
  p->update_graph = opt.update_graph >= 0 ? opt.update_graph : (M <= kUpdGraphAutoRows ? 1 : 0);
  p->update_graph_auto = opt.update_graph < 0;
  p->rollout_kernel = opt.rollout_kernel;
  p->no_update = !opt.update;
  if ((opt.rollout_kernel == 2 || opt.rollout_kernel == 3) && (kind != PPO_NET_LN_BETA || OP > 32))
    return fail(std::string("ppo_create: rollout_kernel=") + (opt.rollout_kernel == 2 ? "valu" : "split") +
                " needs the LayerNorm-Beta agent with obs_dim <= 32");
  if (opt.rollout_kernel == 3 && opt.rollout != PPO_ROLLOUT_AUTO)  // k_rollout_s is a persistent kernel: with rollout=per_step it would never run
    return fail("ppo_create: rollout_kernel=split needs the persistent rollout (rollout=auto, not per_step)");
  int upd_kernel = opt.upd_kernel;
#ifdef PPO_DIAG
  {
    const char* es = getenv("PPO_UPD_SCHED");
    if (es && es[0] >= '0' && es[0] <= '3') p->upd_sched = es[0] - '0';
#ifdef PPO_STAMPS
    if (es) p->upd_sched = atoi(es);  // diagnostic build: bits 4..7 skip stores (ppo_update.hip)
    const char* eg = getenv("PPO_ACT_DIAG");  // diagnostic build: phases of k_act3 to skip (bits, << 8)
    if (eg) p->act_kernel |= atoi(eg) << 8;
#endif
    const char* ea = getenv("PPO_ACT_KERNEL");
    if (ea && (ea[0] == '2' || ea[0] == '4')) p->act_kernel = ea[0] - '0';
    const char* ed = getenv("PPO_DW_FUSED");
    if (ed) p->dw_fused = !(ed[0] == '0');
    const char* ev = getenv("PPO_UPD_KERNEL");
    if (ev && ev[0] == '0') upd_kernel = 1;
    const char* et = getenv("PPO_UPD_TRUNK");
    if (et && (et[0] == '0' || et[0] == '1')) p->upd_trunk_mask = 1 << (et[0] - '0');
    const char* eh = getenv("PPO_UPD2_HOT");
    if (eh) p->upd_hot = atoi(eh);
  }
#endif
  const size_t Mr = ((size_t)M + 63) / 64 * 64;
  const int tiles = (int)(Mr / 64);
  p->tiles_per_block = std::max(1, (tiles + 255) / 256);
  p->nblk = (tiles + p->tiles_per_block - 1) / p->tiles_per_block;
  // ---- the update kernel ----
  {
    // k_upd2 addresses the rollout storage with 32-bit buffer offsets
    const bool fits32 = (double)B * (double)std::max(O, A) * 4.0 < 4294967040.0;
    const int split = !fits32 ? 0 : opt.upd2_split >= 0 ? opt.upd2_split : upd2_split_supported(K) ? kUpd2SplitAuto : 0;
    const char* mfma32_refusal = "ppo_create: upd_mfma=32 / mix needs the LayerNorm-Beta agent at hidden 256";
    if ((opt.upd_mfma == 32 || opt.upd_mfma == 1) && (H != 256 || kind != PPO_NET_LN_BETA)) return fail(mfma32_refusal);
    const char* bx_refusal = "ppo_create: upd_mfma=bx6 needs the LayerNorm-Beta agent at hidden 256 with at most 16 "
                             "heads, or the 64-wide agent's single k_upd2 at OP = 384";
    if (opt.upd_mfma == 6 && !((H == 256 && kind == PPO_NET_LN_BETA) || H == 64)) return fail(bx_refusal);
    if (opt.upd2_split > 0 && (upd_kernel || !fits32 || !upd2_split_supported(K)))
      return fail("ppo_create: upd2_split needs the 64-wide agent with O % 4 == 0, OP = 384 and 32-bit storage offsets");
    // a split-bf16 form is tried into a geometry of its own, so that a form that does not apply leaves
    // nothing behind in the plan's
    UpdGeoOut g = p->upd;
    if (!upd_kernel && fits32 && upd2_supported(K, &p->upd, split) == 0) {
      p->use_upd = p->use_upd2 = true;
      p->upd2_split = split;
      // layer 1 as split-bf16 piece products (the single kernel at cfg2's shape)
      const bool want_bx = opt.upd_mfma == 6 || (opt.upd_mfma == 0 && kUpd2BxAuto);
      g = p->upd;
      if (want_bx && split == 0 && upd2_supported(K, &g, 0, 1) == 0) {
        p->upd = g;
        p->upd_bx = 2;
      } else if (opt.upd_mfma == 6) {
        return fail(bx_refusal);
      }
      const int ut = (M + p->upd.rows - 1) / p->upd.rows;
      // both trunks per workgroup, 2 workgroups per CU x 256 CUs (split form: 3 per CU)
      p->upd_nblk = std::min(ut, split ? 256 * split : 512);
    } else if (opt.upd_mfma == 32 || opt.upd_mfma == 1) {
      p->upd32_mix = opt.upd_mfma == 1;
      if (upd_kernel || upd32_supported(K, sg[1].nh, sg[0].size, sg[1].size, &p->upd, p->upd32_mix) != 0)
        return fail(mfma32_refusal);
      p->use_upd = p->use_upd32 = true;
      p->upd_nblk = std::min((M + p->upd.rows - 1) / p->upd.rows, 256);
    } else if ((opt.upd_mfma == 6 || (opt.upd_mfma == 0 && kUpdBxAuto)) && !upd_kernel &&
               upd_supported(K, sg[1].nh, sg[0].size, sg[1].size, &g, 1) == 0) {
      p->upd = g;
      p->use_upd = true;
      p->upd_bx = 1;
      p->upd_nblk = std::min((M + p->upd.rows - 1) / p->upd.rows, 256);
    } else if (opt.upd_mfma == 6) {
      return fail(bx_refusal);
    } else if (!upd_kernel && upd_supported(K, sg[1].nh, sg[0].size, sg[1].size, &p->upd) == 0) {
      p->use_upd = true;
      const int ut = (M + p->upd.rows - 1) / p->upd.rows;
      p->upd_nblk = std::min(ut, 256);  // 2 workgroups per CU x 256 CUs over the two trunks
    }
  }
  // ---- the critic pass: on split-bf16 products wherever k_upd keeps the critic's W2 pieces (bx6) ----
  p->values_bx = (p->upd_bx == 1 && opt.values_mfma != 0 && rollout_supported(K) == 0) ? 1 : 0;
  if (opt.values_mfma == 6 && !p->values_bx)
    return fail("ppo_create: values_mfma=bx6 needs the LayerNorm-Beta agent at hidden 256 with upd_mfma=bx6 (auto)");
  // ---- launch pairs per minibatch ----
  {
    const bool split_ok = p->use_upd && !p->use_upd2 && !p->use_upd32 && H == 256 && OP <= 32 && p->dw_fused;
    int S = opt.upd_split > 0 ? opt.upd_split : kUpdSplitAuto(M);
    if (!split_ok) {
      if (opt.upd_split > 1)
        return fail("ppo_create: upd_split > 1 needs the fused k_upd + k_dwf path (hidden 256, obs_dim <= 32)");
      S = 1;
    }
    while (S > 1 && M < S * 32 * 64) S /= 2;  // keep >= 64 tiles of 32 rows per launch
    p->msplit = S;
    p->Mq = S == 1 ? M : (((M + S - 1) / S + 31) & ~31);
    while (p->msplit > 1 && (long)(p->msplit - 1) * p->Mq >= M) --p->msplit;  // no empty split
  }
  p->wlds_off = 4 * std::max(sg[0].size, sg[1].size);
  p->wlds_off = (p->wlds_off + 63) & ~63;
  p->lds_bytes = ((size_t)p->wlds_off + 2 * (size_t)H * 16) * sizeof(float);
  // ---- dW ----
  // split-K: ~128 row chunks per trunk (256 workgroups for the two trunks), 16-row multiples
  // (the chunking does not depend on dw_fused, so k_dwf and the two-phase k_dw sum the same chunks)
  // (with upd_split: the geometry of one Mq-row pair; every pair writes its own nchunks partial rows)
  p->dw_slices = dw_slices(p->Mq, H, OP, true);
  if (opt.dw_slices && H == 256 && OP <= 32) p->dw_slices = opt.dw_slices;  // k_dwf geometry only
  p->rows_per_chunk = std::max(64, (((p->Mq + 128 / p->dw_slices - 1) / (128 / p->dw_slices)) + 15) & ~15);
  if (p->use_upd2) p->rows_per_chunk = std::max(32, (((M + 255) / 256) + 31) & ~31);  // k_dw2: both trunks
  if (opt.dw_rows && (!p->use_upd2 || opt.dw_rows % 32 == 0)) p->rows_per_chunk = opt.dw_rows;  // k_dw2: 32-row steps
  p->nchunks = (p->Mq + p->rows_per_chunk - 1) / p->rows_per_chunk;
  {
    const bool rc_ok = p->use_upd && !p->use_upd2 && !p->use_upd32 && kind == PPO_NET_LN_BETA && H == 256 &&
                       OP <= 32 && p->dw_fused && p->dw_dma && p->dw_bx;
    if (opt.h1_handoff == 1 && !rc_ok)
      return fail("ppo_create: h1_handoff=recompute needs the LayerNorm-Beta agent at hidden 256 (obs_dim <= 32) with "
                  "the fused split-bf16 dW (dw_mfma bf16x6/x8/x9)");
    p->h1_recomp = rc_ok && (opt.h1_handoff == 1 || (opt.h1_handoff < 0 && kH1RecomputeAuto));
    // the split-once form covers k_dwf_bx's non-recompute template space (launch_dw's fused dispatch)
    const bool so_ok = !p->use_upd2 && H == 256 && (OP == 16 || OP == 32) && p->dw_fused && p->dw_dma && p->dw_bx &&
                       !p->h1_recomp;
    if (opt.dw_stage == 1 && !so_ok)
      return fail("ppo_create: dw_stage=split_once needs the fused split-bf16 dW (hidden 256, obs_dim <= 32, dw_mfma "
                  "bf16x6/x8/x9) with h1_handoff=store");
    p->dw_so = so_ok && (opt.dw_stage == 1 || (opt.dw_stage < 0 && kDwSplitOnceAuto));
  }
  name_kernels(K, p);
  return 0;
}
