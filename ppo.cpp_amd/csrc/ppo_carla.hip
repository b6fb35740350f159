// ppo_carla.hip — the CaRL CNN agent (include/ppo_carla.h; reference include/carla/carla_model.h:222-318
// with the carla_config.h defaults, training ac_ppo_carla.cpp:529-620). Top to bottom: the agent's
// context, the table of its Linear layers, the forward, the update (loss, backward, clip_grad_norm_,
// Adam), parameter / optimizer I/O, data parallelism, the rollout object's entry points. The kernels of
// the layers live in ppo_carla_conv / _tail / _ln / _grad.hip (ppo_carla_units.hpp).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ppo_carla_units.hpp"
#include "ppo_dist.hpp"

// ------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------
// The forward's buffers (activations, split-K partials, conv1's weight table, the tail's barrier, the
// LayerNorm z / stat) are the base CarlaFwdBufs (ppo_carla_internal.hpp): the agent's own set, which
// ppo_carla_forward and ppo_carla_update use; an act lane brings its own to carla_forward.
struct ppo_carla : CarlaFwdBufs, CarlaGradBufs {
  ppo_carla_config cfg;
  ppo_carla_layout2 L;  // arch all zero: the offsets of ppo_carla_layout
  CarlaNet net;         // the Linear layers (carla_net_init)
  int device = 0;
  hipStream_t stream = nullptr;
  float* P = nullptr;
  // recorded after every parameter change (carla_params_mark); act lanes wait for it
  hipEvent_t params_ev = nullptr;
  // training state (allocated on the first ppo_carla_update)
  bool train_ready = false;
  float *G = nullptr, *m = nullptr, *v = nullptr;        // [P]
  float* dact[PPO_CARLA_NCONV - 1] = {};                 // d(conv1..conv5 outputs), masked
  float* dhead = nullptr;                                // [B][2A]; the other activations' gradients: CarlaGradBufs
  float *lp = nullptr, *ent = nullptr, *rowstat = nullptr;                    // rowstat [B][8]
  float *part = nullptr;                                 // wgrad partials
  size_t part_floats = 0;
  float* small = nullptr;  // scalars, tensor table and norm slices (carla_train_init)
  long step = 0;
  // Adam options (ppo_carla_set_adam): exactly (0.9, 0.999, 0) launches k_carla_adam, anything else k_carla_adam_opt
  double beta1 = 0.9, beta2 = 0.999, weight_decay = 0.0;
  // conv1 / conv2 kernels: 2 packed conv1 taps (k_conv_img3), 1 LDS-staged (k_conv_img2 and the staged
  // wgrad / dgrad kernels), 0 generic (create option conv1=packed|staged|generic; PPO_CARLA_CONV1 in the
  // diagnostic build). The backward's staged kernels run for 1 and 2.
  int conv_img = kConv1Auto;
  // conv1 (raw-byte input) as split-bf16 products on bf16 MFMAs (create option conv1_mfma=bx3|f32):
  // k_wgrad_img2<.., BX> and k_conv_img3<.., BX>
  int c1bx = kConv1BxAuto;
  // conv2's input gradient: 1 k_dgrad_q (quad classes as GEMM columns), 0 k_dgrad_s2 (create option
  // conv_dgrad=quad|staged; both need conv1=staged|packed)
  int dgrad_q = kDgradQuadAuto;
  // conv2's weight gradient: 1 k_wgrad_t (LDS-staged tiles), 0 k_wgrad (create option conv_wgrad=tiled|generic)
  int wgrad_t = kWgradTiledAuto;
  // conv2's forward: 1 k_conv_t (LDS-staged input patches), 0 k_conv (create option conv_fwd=tiled|generic)
  int conv_t = kConvTiledAuto;
  // conv6's input gradient: 1 dense GEMM + col2im (create option deep_dgrad=col|gather)
  int dgrad_col = kDgradColAuto;
  // create option wgrad_group_bytes (tests): the generic fp32 k_wgrad runs its samples in groups whose
  // input stays below this many bytes (0: kWgradFar, the limit of its 32-bit buffer offsets)
  long wgrad_group = 0;
  float *dcol = nullptr, *wt = nullptr, *zbias = nullptr;  // carla_train_init
  // MLP tail for n <= kTailMaxN: 1 (default) one launch per stage, 0 one cooperative launch (a grid
  // barrier between stages: slower here, a cooperative launch costs more than the launches it
  // saves), 2 one k_conv / k_conv_fin pair per layer
  int tail_mode = 1;
  // data parallelism (ppo_carla_comm_init): one RCCL communicator, any world >= 1
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1;
  // LayerNorm agents: the column pass's chunk sums (carla_train_init)
  float* lnpart = nullptr;
  size_t lnpart_floats = 0;
  // positional agents (L.conv_ic[0] == L.C + 2): the row / column sums of dZ1 per sample chunk (carla_train_init)
  float* pospart = nullptr;
  size_t pospart_floats = 0;
};

// use_positional_encoding: conv1's filters hold two more channels than the image has
static inline bool carla_pos(const ppo_carla_layout2& L) { return L.conv_ic[0] != L.C; }
// the channels convolution i reads from memory (conv1: the image's, also for a positional agent)
static inline int carla_in_c(const ppo_carla_layout2& L, int i) { return i ? L.conv_ic[i] : L.C; }

static int carla_alloc(float** p, size_t n) {
  if (hipMalloc((void**)p, (n ? n : 1) * sizeof(float)) != hipSuccess) return -2;
  return hipMemset(*p, 0, (n ? n : 1) * sizeof(float)) == hipSuccess ? 0 : -2;
}

// The Linear layers in forward order: state_linear (carla_model.h:238), linear (:240), value_head on
// [features | value_measurements] (:276-277), policy_head on features (:279). Concatenations are strides.
static void carla_net_init(const ppo_carla_layout2& L, CarlaNet* net) {
  using F = CarlaFwdBufs;
  const long FW = 256 + L.NV;
  const CarlaLayer t[kCarlaLayers] = {
      // in, out, in_stride, out_stride, IN, OUT, w, b, relu, ln, g, be, stage, to_value
      {kBufMeas, kBufS1, L.NM, 256, L.NM, 256, L.st_w[0], L.st_b[0], 1, F::kLnS1, L.st_g[0], L.st_be[0], 0, false},
      {kBufS1, kBufState, 256, 1280, 256, 256, L.st_w[1], L.st_b[1], 1, F::kLnS2, L.st_g[1], L.st_be[1], 1, false},
      {kBufEnc, kBufL1, 1280, 512, 1280, 512, L.lin_w[0], L.lin_b[0], 1, F::kLnL1, L.lin_g[0], L.lin_be[0], 2, false},
      {kBufL1, kBufFeat, 512, FW, 512, 256, L.lin_w[1], L.lin_b[1], 1, F::kLnFeat, L.lin_g[1], L.lin_be[1], 3, false},
      {kBufFeat, kBufV1, FW, 256, (int)FW, 256, L.v_w[0], L.v_b[0], 1, F::kLnV1, L.v_g[0], L.v_be[0], 4, false},
      {kBufV1, kBufV2, 256, 256, 256, 256, L.v_w[1], L.v_b[1], 1, F::kLnV2, L.v_g[1], L.v_be[1], 5, false},
      {kBufV2, kBufVal, 256, 1, 256, 1, L.v_w[2], L.v_b[2], 0, -1, -1, -1, 6, true},
      {kBufFeat, kBufP1, FW, 256, 256, 256, L.pi_w[0], L.pi_b[0], 1, F::kLnP1, L.pi_g[0], L.pi_be[0], 4, false},
      {kBufP1, kBufP2, 256, 256, 256, 256, L.pi_w[1], L.pi_b[1], 1, F::kLnP2, L.pi_g[1], L.pi_be[1], 5, false},
  };
  int k = 0;
  for (int st = 0; k < kCarlaLayers; ++st)  // stable: k_carla_tail needs non-decreasing stages
    for (int i = 0; i < kCarlaLayers; ++i)
      if (t[i].stage == st) net->tail_order[k++] = i;
  std::copy(t, t + kCarlaLayers, net->layer);
}

// Convolution i of the layout on n samples, for each of its three launchers. Its input (the image or
// act[i - 1]) is contiguous; out / dz may be strided (conv6 writes columns 0..1023 of enc).
static ConvArgs conv_args(const ppo_carla_layout2& L, int i, const float* P, const float* in_f, const uint8_t* in_u8,
                          float* out, long out_stride, int relu, int n, float* ksplit) {
  const int ic = carla_in_c(L, i);
  ConvArgs a{in_f, in_u8, (long)ic * L.conv_ih[i] * L.conv_iw[i], ic, L.conv_ih[i],
             L.conv_iw[i], P + L.conv_w[i], P + L.conv_b[i], out, out_stride, L.conv_oc[i], L.conv_oh[i],
             L.conv_ow[i], L.conv_k[i], L.conv_s[i], relu, n, ksplit, 0};
  if (i == 0 && carla_pos(L)) {  // the raw bytes against the image channels of the wider filters
    a.wstride = L.conv_ic[0] * L.conv_k[0] * L.conv_k[0];
    a.xscale = 1.0f;
  }
  return a;
}
static WgradArgs wgrad_args(const ppo_carla_layout2& L, int i, const float* dz, long dz_stride, const float* x_f,
                            const uint8_t* x_u8, int n, long group_bytes) {
  const int ic = carla_in_c(L, i);
  WgradArgs a{dz, dz_stride, L.conv_oc[i], L.conv_oh[i] * L.conv_ow[i], L.conv_ow[i], x_f, x_u8,
              (long)ic * L.conv_ih[i] * L.conv_iw[i], ic, L.conv_ih[i], L.conv_iw[i],
              L.conv_k[i], L.conv_s[i], n, ic * L.conv_k[i] * L.conv_k[i], 0, nullptr, group_bytes};
  if (i == 0 && carla_pos(L)) {
    a.wstride = L.conv_ic[0] * L.conv_k[0] * L.conv_k[0];
    a.xscale = 1.0f;
  }
  return a;
}
static DgradArgs dgrad_args(const ppo_carla_layout2& L, int i, const float* P, const float* dz, long dz_stride,
                            const float* x, float* dx, int n) {
  const long xs = (long)L.conv_ic[i] * L.conv_ih[i] * L.conv_iw[i];
  return DgradArgs{dz, dz_stride, P + L.conv_w[i], L.conv_ic[i], x, xs, dx, xs, L.conv_ic[i], L.conv_ih[i],
                   L.conv_iw[i], L.conv_oc[i], L.conv_oh[i], L.conv_ow[i], L.conv_k[i], L.conv_s[i], n, 0};
}

int carla_fwd_alloc(const ppo_carla_t* c, size_t B, CarlaFwdBufs* fb) {
  const ppo_carla_layout2& L = c->L;
  int rc = 0;
  for (int i = 0; i < PPO_CARLA_NCONV - 1; ++i)
    rc |= carla_alloc(&fb->act[i], B * L.conv_oc[i] * L.conv_oh[i] * L.conv_ow[i]);
  rc |= carla_alloc(&fb->enc, B * 1280);
  rc |= carla_alloc(&fb->s1, B * 256);
  rc |= carla_alloc(&fb->l1, B * 512);
  rc |= carla_alloc(&fb->feat, B * (256 + L.NV));
  rc |= carla_alloc(&fb->v1, B * 256);
  rc |= carla_alloc(&fb->v2, B * 256);
  rc |= carla_alloc(&fb->val, B);
  rc |= carla_alloc(&fb->p1, B * 256);
  rc |= carla_alloc(&fb->p2, B * 256);
  rc |= carla_alloc(&fb->hpre, B * 2 * L.A);
  {  // the largest split-K partial buffer of the forward's layers
    size_t m = 0;
    auto need = [&](int Kt, int P, int OC) {
      const int Z = conv_split_z(Kt, P);
      if (Z > 1) m = std::max(m, (size_t)Z * B * P * OC);
    };
    for (int i = 1; i < PPO_CARLA_NCONV; ++i)
      need(L.conv_ic[i] * L.conv_k[i] * L.conv_k[i], L.conv_oh[i] * L.conv_ow[i], L.conv_oc[i]);
    for (const CarlaLayer& e : c->net.layer) need(e.IN, 1, e.OUT);
    if (m) rc |= carla_alloc(&fb->ksplit, m);
  }
  rc |= carla_alloc(&fb->c1w, (size_t)img3_blocks(L.C, L.conv_k[0]) * 256);
  if (carla_pos(L)) rc |= carla_alloc(&fb->posb, (size_t)L.conv_oc[0] * (L.conv_oh[0] + L.conv_ow[0]));
  rc |= carla_alloc(reinterpret_cast<float**>(&fb->tail_bar), 1);
  fb->tail_count = 0;
  {  // pre-activation and statistics buffers of the normalised layers
    auto ln = [&](int k, int F, long g, long be) {
      if (g < 0) return;
      fb->ln[k].F = F;
      fb->ln[k].g = g;
      fb->ln[k].be = be;
      rc |= carla_alloc(&fb->ln[k].z, B * F);
      rc |= carla_alloc(&fb->ln[k].stat, B * 2);
      fb->any_ln = true;
    };
    for (int i = 0; i < PPO_CARLA_NCONV; ++i)
      ln(CarlaFwdBufs::kLnConv + i, L.conv_oc[i] * L.conv_oh[i] * L.conv_ow[i], L.conv_g[i], L.conv_be[i]);
    for (const CarlaLayer& e : c->net.layer)
      if (e.ln >= 0) ln(e.ln, e.OUT, e.g, e.be);
  }
  return rc ? -2 : 0;
}

void carla_fwd_free(CarlaFwdBufs* fb) {
  float* bufs[] = {fb->enc, fb->s1, fb->l1,   fb->feat,   fb->v1,  fb->v2,
                   fb->val, fb->p1, fb->p2,   fb->hpre,   fb->ksplit, fb->c1w, fb->posb, reinterpret_cast<float*>(fb->tail_bar)};
  for (float* b : bufs)
    if (b) (void)hipFree(b);
  for (float* b : fb->act)
    if (b) (void)hipFree(b);
  for (auto& l : fb->ln) {
    if (l.z) (void)hipFree(l.z);
    if (l.stat) (void)hipFree(l.stat);
  }
  *fb = CarlaFwdBufs{};
}

extern "C" int ppo_carla_destroy(ppo_carla_t* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) (void)ncclCommDestroy(c->comm);
  float* bufs[] = {c->P,  c->G,   c->m,       c->v,    c->dhead, c->lp,   c->ent,
                   c->rowstat, c->part, c->small, c->dcol, c->wt,  c->zbias};
  for (float* b : bufs)
    if (b) (void)hipFree(b);
  for (float* b : c->d)
    if (b) (void)hipFree(b);
  carla_fwd_free(c);
  for (float* b : c->dact)
    if (b) (void)hipFree(b);
  if (c->lnpart) (void)hipFree(c->lnpart);
  if (c->pospart) (void)hipFree(c->pospart);
  if (c->params_ev) (void)hipEventDestroy(c->params_ev);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

extern "C" int ppo_carla_create(const ppo_carla_config* cfg, int device, ppo_carla_t** out) {
  return ppo_carla_create_ex(cfg, device, nullptr, out);
}

extern "C" int ppo_carla_create_ex(const ppo_carla_config* cfg, int device, const char* options, ppo_carla_t** out) {
  return ppo_carla_create2(cfg, nullptr, device, options, out);
}

extern "C" int ppo_carla_create2(const ppo_carla_config* cfg, const ppo_carla_arch* arch, int device,
                                 const char* options, ppo_carla_t** out) {
  return ppo_carla_create3(cfg, arch, 0, device, options, out);
}

extern "C" int ppo_carla_create3(const ppo_carla_config* cfg, const ppo_carla_arch* arch, int pos_enc, int device,
                                 const char* options, ppo_carla_t** out) {
  if (!cfg || !out) return ppo_fail("ppo_carla_create: null argument", -1);
  if (pos_enc != 0 && pos_enc != 1)
    return ppo_fail("ppo_carla_create3: pos_enc must be 0 or 1 (use_positional_encoding), got " +
                    std::to_string(pos_enc), -1);
  int conv_img = kConv1Auto;
  int tail_mode = 1;
  const char* tail_given = nullptr;
  int c1bx = kConv1BxAuto;
  int dgrad_q = kDgradQuadAuto;
  int wgrad_t = kWgradTiledAuto;
  int conv_t = kConvTiledAuto;
  int dgrad_col = kDgradColAuto;
  long wgrad_group = 0;
  if (options && *options) {  // comma-separated key=value
    std::string rest(options);
    while (!rest.empty()) {
      const size_t cpos = rest.find(',');
      const std::string o = rest.substr(0, cpos);
      rest = cpos == std::string::npos ? std::string() : rest.substr(cpos + 1);
      if (o == "conv1=packed") conv_img = 2;
      else if (o == "conv1=staged") conv_img = 1;
      else if (o == "conv1=generic") conv_img = 0;
      else if (o == "tail=fused") tail_mode = 0, tail_given = "tail=fused";
      else if (o == "tail=staged") tail_mode = 1, tail_given = "tail=staged";
      else if (o == "tail=layers") tail_mode = 2;
      else if (o == "conv1_mfma=bx3") c1bx = 1;
      else if (o == "conv1_mfma=f32") c1bx = 0;
      else if (o == "conv1_mfma=auto") c1bx = kConv1BxAuto;
      else if (o == "conv_dgrad=quad") dgrad_q = 1;
      else if (o == "conv_dgrad=staged") dgrad_q = 0;
      else if (o == "conv_dgrad=auto") dgrad_q = kDgradQuadAuto;
      else if (o == "conv_wgrad=tiled") wgrad_t = 1;
      else if (o == "conv_wgrad=generic") wgrad_t = 0;
      else if (o == "conv_wgrad=auto") wgrad_t = kWgradTiledAuto;
      else if (o == "conv_fwd=tiled") conv_t = 1;
      else if (o == "conv_fwd=generic") conv_t = 0;
      else if (o == "conv_fwd=auto") conv_t = kConvTiledAuto;
      else if (o == "deep_dgrad=col") dgrad_col = 1;
      else if (o == "deep_dgrad=gather") dgrad_col = 0;
      else if (o == "deep_dgrad=auto") dgrad_col = kDgradColAuto;
      else if (o.rfind("wgrad_group_bytes=", 0) == 0 && o.size() > 18 && o.size() <= 28 &&
               o.find_first_not_of("0123456789", 18) == std::string::npos)
        wgrad_group = atol(o.c_str() + 18);
      else return ppo_fail("ppo_carla_create_ex: unknown option " + o, -1);
    }
  }
  // LayerNorm variants: refusals that need no device
  const bool any_ln = arch && (arch->encoder_ln || arch->mlp_ln);
  if (arch && (arch->encoder_ln < 0 || arch->encoder_ln > 1))
    return ppo_fail("ppo_carla_create2: encoder_ln must be 0 (roach) or 1 (roach_ln); roach_ln2 is not built", -1);
  if (arch && arch->encoder_ln && (cfg->bev_h != 192 || cfg->bev_w != 192))
    return ppo_fail("ppo_carla_create2: the roach_ln encoder needs a 192 x 192 bev: the reference hard-codes its "
                    "LayerNorm shapes ([8, 94, 94] ... [256, 2, 2], carla_model.h:45-62)", -1);
  if (any_ln && tail_given)
    return ppo_fail(std::string("ppo_carla_create2: option ") + tail_given +
                    " cannot be used by a LayerNorm agent (its forward runs one launch per layer, tail=layers)", -1);
  if (any_ln) tail_mode = 2;
  if (int rc = ppo_runtime_check()) return rc;
  ppo_carla_layout2 L{};  // unused table entries stay zero
  if (ppo_carla_layout2_init_pos(&L, cfg->obs_channels, cfg->bev_h, cfg->bev_w, cfg->num_measurements,
                                 cfg->num_value_measurements, cfg->action_dim, arch, pos_enc) != 0)
    return ppo_fail("ppo_carla_create: the roach encoder needs a bev that ends at 256 x 2 x 2 (n_flatten = 1024, "
                    "carla_model.h:110)", -1);
  if (cfg->max_batch <= 0) return ppo_fail("ppo_carla_create: max_batch must be positive", -1);
  if (pos_enc && (L.conv_oh[0] > kPosMaxOH || L.conv_ow[0] > kPosMaxOW))
    return ppo_fail("ppo_carla_create3: positional encoding needs a first convolution of at most " +
                    std::to_string(kPosMaxOH) + " x " + std::to_string(kPosMaxOW) + " outputs", -1);
  if ((long)L.C * L.conv_k[0] * L.conv_k[0] > kMaxKTab || 1280 > kMaxKTab)
    return ppo_fail("ppo_carla_create: too many input channels", -1);
  if (hipSetDevice(device) != hipSuccess) return ppo_fail("ppo_carla_create: hipSetDevice failed", -2);
  ppo_carla_t* c = new ppo_carla_t();
  c->cfg = *cfg;
  c->L = L;
  carla_net_init(L, &c->net);
  c->device = device;
  c->conv_img = conv_img;
  c->tail_mode = tail_mode;
  c->c1bx = c1bx;
  c->dgrad_q = dgrad_q;
  c->wgrad_t = wgrad_t;
  c->conv_t = conv_t;
  c->dgrad_col = dgrad_col;
  c->wgrad_group = wgrad_group;
#ifdef PPO_DIAG
  if (const char* e = getenv("PPO_CARLA_CONV1")) c->conv_img = e[0] - '0';
#endif
  int rc = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess ? 0 : -2;
  rc |= hipEventCreateWithFlags(&c->params_ev, hipEventDisableTiming) == hipSuccess ? 0 : -2;
  rc |= carla_alloc(&c->P, L.P);
  rc |= carla_fwd_alloc(c, (size_t)cfg->max_batch, c);
  if (rc || hipDeviceSynchronize() != hipSuccess) {
    ppo_carla_destroy(c);
    return ppo_fail("ppo_carla_create: device allocation failed", -2);
  }
  *out = c;
  return 0;
}

static_assert(offsetof(ppo_carla_layout, sg_b) == offsetof(ppo_carla_layout2, sg_b) &&
                  offsetof(ppo_carla_layout, ntensors) == offsetof(ppo_carla_layout, sg_b) + sizeof(long),
              "ppo_carla_layout2 must begin with ppo_carla_layout's fields");

extern "C" int ppo_carla_get_layout(const ppo_carla_t* c, ppo_carla_layout* out) {
  if (!c || !out) return ppo_fail("ppo_carla_get_layout: null argument", -1);
  if (c->any_ln)
    return ppo_fail("ppo_carla_get_layout: ppo_carla_layout cannot describe a LayerNorm agent's tensors; use "
                    "ppo_carla_get_layout2", -1);
  if (carla_pos(c->L))
    return ppo_fail("ppo_carla_get_layout: ppo_carla_layout cannot describe a positional agent's cnn.0.weight "
                    "([8, C + 2, 5, 5]); use ppo_carla_get_layout2", -1);
  // the default arch's layout2 holds ppo_carla_layout's fields with the same values, in the same order
  // up to the tensor table
  const ppo_carla_layout2& L = c->L;
  memcpy(out, &L, offsetof(ppo_carla_layout, ntensors));
  out->ntensors = L.ntensors;
  for (int t = 0; t < PPO_CARLA_MAX_TENSORS; ++t) {
    out->t_off[t] = L.t_off[t];
    out->t_len[t] = L.t_len[t];
    out->t_grad[t] = L.t_grad[t];
  }
  return 0;
}

extern "C" int ppo_carla_get_layout2(const ppo_carla_t* c, ppo_carla_layout2* out) {
  if (!c || !out) return ppo_fail("ppo_carla_get_layout2: null argument", -1);
  *out = c->L;
  return 0;
}

extern "C" int ppo_carla_load_params(ppo_carla_t* c, const float* host, long n) {
  if (!c || !host) return ppo_fail("ppo_carla_load_params: null argument", -1);
  if (n != c->L.P) return ppo_fail("ppo_carla_load_params: expected " + std::to_string(c->L.P) + " floats", -1);
  if (hipSetDevice(c->device) != hipSuccess ||
      hipMemcpyAsync(c->P, host, sizeof(float) * n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    return ppo_fail("ppo_carla_load_params: copy failed", -2);
  return carla_params_mark(c, c->stream);
}

extern "C" int ppo_carla_forward(ppo_carla_t* c, int n, const uint8_t* bev, const float* meas, const float* vmeas,
                                 int sample_type, const float* action_in, long env_base, long step_id, float* action,
                                 float* logprob, float* entropy, float* value, float* alpha, float* beta,
                                 void* stream) {
  if (!c || !bev || !meas || (!vmeas && c->L.NV > 0)) return ppo_fail("ppo_carla_forward: null argument", -1);
  if (n <= 0) return 0;
  if (n > c->cfg.max_batch) return ppo_fail("ppo_carla_forward: n exceeds max_batch", -1);
  if (sample_type < PPO_CARLA_SAMPLE || sample_type > PPO_CARLA_ROACH)
    return ppo_fail("Unsupported sample type used. Sample type: " + std::to_string(sample_type), -1);
  if (sample_type == PPO_CARLA_GIVEN && !action_in) return ppo_fail("ppo_carla_forward: GIVEN needs action_in", -1);
  if (hipSetDevice(c->device) != hipSuccess) return ppo_fail("ppo_carla_forward: hipSetDevice failed", -2);
  return carla_forward(c, *c, stream ? (hipStream_t)stream : c->stream, n, bev, meas, vmeas, sample_type, action_in,
                       env_base, step_id, action, logprob, entropy, value, alpha, beta);
}

int carla_forward(const ppo_carla_t* c, CarlaFwdBufs& fb, hipStream_t s, int n, const uint8_t* bev, const float* meas,
                  const float* vmeas, int sample_type, const float* action_in, long env_base, long step_id,
                  float* action, float* logprob, float* entropy, float* value, float* alpha, float* beta) {
  const ppo_carla_layout2& L = c->L;
  const float* P = c->P;
  if (carla_pos(L))  // conv1's row / column tables from its current weights (as k_conv1_wprep's table)
    (void)launch_pos_bias(L.conv_oc[0], L.conv_ic[0], L.C, L.conv_k[0], L.conv_s[0], L.IH, L.IW, P + L.conv_w[0], fb.posb,
                          fb.posb + (size_t)L.conv_oc[0] * L.conv_oh[0], s);
  auto conv = [&](ConvArgs a) {
    if (a.in_u8 && fb.posb) {
      a.rowb = fb.posb;
      a.colb = fb.posb + (size_t)L.conv_oc[0] * L.conv_oh[0];
    }
    a.wprep = fb.c1w;
    a.bx = c->c1bx;
    a.tiled = c->conv_t;
    return launch_conv(a, s, c->conv_img);
  };
  auto linear = [&](const float* in, long in_stride, int IN, long w, long b, float* out, long out_stride, int OUT,
                    int relu) {
    return conv(ConvArgs{in, nullptr, in_stride, IN, 1, 1, P + w, P + b, out, out_stride, OUT, 1, 1, 1, 1, relu, n,
                         fb.ksplit, 0});
  };
  // a normalised layer: the pre-activation goes to ln[k].z, k_carla_ln writes the layer's output
  auto norm = [&](int k, float* out, long out_stride) {
    const CarlaFwdBufs::Ln& l = fb.ln[k];
    launch_ln_fwd(n, l.F, l.z, l.F, P + l.g, P + l.be, out, out_stride, l.stat, s);
  };
  int rc = 0;
  const bool fused_tail = c->tail_mode != 2 && n <= kTailMaxN;
  ConvArgs c6{};
  int c6_Z = 1;
  // cnn (carla_model.h:66-78, :236): conv1 reads the uint8 image, conv6 writes linear-input columns 0..1023
  const uint8_t* img = bev;
  const float* cur = nullptr;
  for (int i = 0; i < PPO_CARLA_NCONV; ++i) {
    const bool last = i == PPO_CARLA_NCONV - 1;
    float* out = last ? fb.enc : fb.act[i];
    const long out_stride = last ? 1280 : (long)L.conv_oc[i] * L.conv_oh[i] * L.conv_ow[i];
    const CarlaFwdBufs::Ln& l = fb.ln[CarlaFwdBufs::kLnConv + i];
    if (last && fused_tail) {  // conv6's split-K finish moves into the tail's stage 0
      c6 = conv_args(L, i, P, cur, nullptr, out, out_stride, 1, n, fb.ksplit);
      rc |= launch_conv(c6, s, c->conv_img, false, &c6_Z);
    } else if (l.F) {  // roach_ln: conv -> LayerNorm([OC, OH, OW]) -> ReLU
      rc |= conv(conv_args(L, i, P, cur, img, l.z, l.F, 0, n, fb.ksplit));
      norm(CarlaFwdBufs::kLnConv + i, out, out_stride);
    } else {
      rc |= conv(conv_args(L, i, P, cur, img, out, out_stride, 1, n, fb.ksplit));
    }
    img = nullptr;
    cur = out;
  }
  const HeadArgs h{P,          L.mu_w, L.mu_b,   L.sg_w,    L.sg_b,    L.hi,    L.lo,
                   fb.p2,      fb.val, n,        L.A,       sample_type, c->cfg.beta_min, action_in,
                   c->cfg.seed, c->cfg.rank, env_base, step_id, action, logprob, entropy, value, alpha, beta,
                   fb.hpre};
  if (fused_tail) {
    if (rc) return ppo_fail("ppo_carla_forward: no convolution kernel for this shape", -1);
    return launch_carla_tail(c->net, fb, P, n, c6, c6_Z, meas, vmeas, L.NM, L.NV, value, h, c->tail_mode == 0, s);
  }
  // one k_conv (+ k_conv_fin, + k_carla_ln) per layer
  for (const CarlaLayer& e : c->net.layer) {
    const float* in = e.in == kBufMeas ? meas : carla_buf(fb, e.in);
    float* out = carla_buf(fb, e.out);
    if (e.ln >= 0 && fb.ln[e.ln].F) {
      rc |= linear(in, e.in_stride, e.IN, e.w, e.b, fb.ln[e.ln].z, e.OUT, e.OUT, 0);
      norm(e.ln, out, e.out_stride);
    } else {
      rc |= linear(in, e.in_stride, e.IN, e.w, e.b, out, e.out_stride, e.OUT, e.relu);
    }
    if (e.out == kBufFeat && L.NV > 0) launch_carla_pack(vmeas, fb.feat, n, L.NV, s);
  }
  if (rc) return ppo_fail("ppo_carla_forward: no convolution kernel for this shape", -1);
  launch_carla_head(h, s);
  if (hipGetLastError() != hipSuccess) return ppo_fail("ppo_carla_forward: launch failed", -2);
  return 0;
}

// ==========================================================================================
// Training (ac_ppo_carla.cpp:529-620): the loss, backward through every layer (ppo_carla_grad.hip,
// ppo_carla_ln.hip), clip_grad_norm_, Adam.
// ==========================================================================================
namespace {

// the same statistics in the distributed order of ac_ppo_carla.cpp:561-580, one block each:
// phase 0: out[0] = local mean; phase 1: out[2] = sum (adv - out[0])^2 about the (all-reduced) mean
__global__ __launch_bounds__(256) void k_carla_adv_part(const float* __restrict__ adv, int n, float* __restrict__ out,
                                                        int phase) {
  __shared__ float red[256];
  float s = 0.f;
  if (phase == 0) {
    for (int i = threadIdx.x; i < n; i += 256) s += adv[i];
  } else {
    const float mean = out[0];
    for (int i = threadIdx.x; i < n; i += 256) s += (adv[i] - mean) * (adv[i] - mean);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (phase == 0) out[0] = red[0] / (float)n;
    else out[2] = red[0];
  }
}
// out[1] = sqrt(sum of squares over all ranks / (world * n - 1))
__global__ void k_carla_adv_fin(float* __restrict__ out, float denom) {
  if (threadIdx.x == 0) out[1] = sqrtf(out[2] / denom);
}

// minibatch advantage mean / std (Bessel), one block, fixed summation order
__global__ __launch_bounds__(256) void k_carla_advstats(const float* __restrict__ adv, int n, float* __restrict__ out) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += adv[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const float mean = red[0] / (float)n;
  __syncthreads();
  float q = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) q += (adv[i] - mean) * (adv[i] - mean);
  red[threadIdx.x] = q;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = mean;
    out[1] = sqrtf(red[0] / (float)(n - 1));
  }
}

struct HeadBwdArgs {
  const float* P;
  long hi, lo;
  const float* hpre;  // [n][2A]
  const float* actions;
  const float *lp, *ent, *val, *old_logp, *adv, *ret, *old_v;
  const float* advstat;  // mean, std
  int n, A;
  float beta_min, clip, ent_coef, vf_coef;
  int norm_adv, clip_vloss;
  float* dhead;    // [n][2A]
  float* dval;     // [n]
  float* rowstat;  // [n][8]
};

// loss -> d(dist_mu, dist_sigma pre-activations), d(value); the terms of the minibatch stats
__global__ __launch_bounds__(64) void k_carla_head_bwd(HeadBwdArgs h) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= h.n) return;
  const float invM = 1.0f / (float)h.n;
  const float am = h.norm_adv ? h.advstat[0] : 0.f, as = h.norm_adv ? h.advstat[1] : 0.f;
  const PpoSurrogate sl = ppo_surrogate(h.lp[r], h.old_logp[r], h.adv[r], h.norm_adv, am, as, h.clip, invM, h.ent_coef);
  const PpoValueLoss vl = ppo_value_loss(h.val[r], h.ret[r], h.old_v[r], h.clip, h.clip_vloss, h.vf_coef, invM);
  const float g_logp = sl.g_logp, g_ent = sl.g_ent;
  const float hi = h.P[h.hi], lo = h.P[h.lo];
  for (int ai = 0; ai < h.A; ++ai) {
    const float pm = h.hpre[(long)r * 2 * h.A + ai], ps = h.hpre[(long)r * 2 * h.A + h.A + ai];
    const float al = softplusf_(pm) + h.beta_min, be = softplusf_(ps) + h.beta_min;
    const float sv = beta_unit_from_action(h.actions[(long)r * h.A + ai], lo, hi);
    const float ab = al + be;
    const BetaGrad bg = beta_grad(al, be, sv, digammaf_(al), digammaf_(be), digammaf_(ab), trigammaf_(al), trigammaf_(be),
                                  trigammaf_(ab));
    h.dhead[(long)r * 2 * h.A + ai] = (g_logp * bg.dla + g_ent * bg.dea) * softplus_d(pm);
    h.dhead[(long)r * 2 * h.A + h.A + ai] = (g_logp * bg.dlb + g_ent * bg.deb) * softplus_d(ps);
  }
  h.dval[r] = vl.g_v;
  float* st = h.rowstat + (long)r * 8;
  st[0] = sl.pg;
  st[1] = vl.term;
  st[2] = h.ent[r];
  st[3] = sl.okl;
  st[4] = sl.kl;
  st[5] = sl.clipfrac;
}

// row means of the stats, one block, fixed order: pg, 0.5*v, entropy, old_kl, kl, clipfrac
__global__ __launch_bounds__(256) void k_carla_stats(const float* __restrict__ rowstat, int n, float* __restrict__ out) {
  __shared__ float red[6][256];
  float a[6] = {0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < n; i += 256)
    for (int k = 0; k < 6; ++k) a[k] += rowstat[(long)i * 8 + k];
  for (int k = 0; k < 6; ++k) red[k][threadIdx.x] = a[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w)
      for (int k = 0; k < 6; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 6) out[threadIdx.x] = red[threadIdx.x][0] / (float)n * (threadIdx.x == 1 ? 0.5f : 1.0f);
}

constexpr int kNormSplit = 32;

// per-tensor sums of squares of the gradient, kNormSplit slices per tensor (blockIdx.y)
__global__ __launch_bounds__(256) void k_carla_tnorm(const float* __restrict__ G, const long* __restrict__ off,
                                                     const long* __restrict__ len, float* __restrict__ part) {
  __shared__ float red[256];
  const int t = blockIdx.x, sp = blockIdx.y;
  const long n = len[t], per = (n + kNormSplit - 1) / kNormSplit, b = sp * per, e = b + per < n ? b + per : n;
  float q = 0.f;
  for (long i = b + threadIdx.x; i < e; i += 256) {
    const float x = G[off[t] + i];
    q += x * x;
  }
  red[threadIdx.x] = q;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[t * kNormSplit + sp] = red[0];
}

// clip_grad_norm_ (clip_grad.h): norm_t = ||g_t|| (slices added in order), total = ||(norm_t)||,
// coef = clamp(max_norm / (total + 1e-6), max = 1); out = {total, coef}
__global__ void k_carla_tsum(const float* __restrict__ part, int nt, float max_norm, float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  float tot = 0.f;
  for (int t = 0; t < nt; ++t) {
    float q = 0.f;
    for (int sp = 0; sp < kNormSplit; ++sp) q += part[t * kNormSplit + sp];
    const float nrm = sqrtf(q);
    tot += nrm * nrm;
  }
  const float total = sqrtf(tot);
  const float coef = max_norm / (total + 1e-6f);
  out[0] = total;
  out[1] = coef > 1.0f ? 1.0f : coef;
}

struct CarlaAdamArgs {
  float *P, *G, *m, *v;
  long begin, n;        // trainable range [begin, begin + n)
  const float* clip;    // {total, coef} from k_carla_tsum
  float step_size, sbc2, eps;
};

__global__ __launch_bounds__(256) void k_carla_adam(CarlaAdamArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const long p = a.begin + i;
  const float gv = a.G[p] * a.clip[1];
  const float m = a.m[p] * 0.9f + gv * 0.1f;
  const float v = a.v[p] * 0.999f + gv * gv * 0.001f;
  a.m[p] = m;
  a.v[p] = v;
  a.P[p] = a.P[p] - a.step_size * (m / (sqrtf(v) / a.sbc2 + a.eps));
}

// Adam with the optimizer's options as arguments (ppo_carla_set_adam): LibTorch's Adam::step after
// clip_grad_norm_, with coupled L2 (g += wd * p before the moments; not AdamW). k_carla_adam keeps the
// options (0.9, 0.999, 0) compiled in and stays the launch for exactly those.
struct CarlaAdamOptArgs {
  float *P, *G, *m, *v;
  long begin, n;        // trainable range [begin, begin + n)
  long head, nvec;      // scalar elements before the first 16-byte boundary, then float4 groups, then the rest
  const float* clip;    // {total, coef} from k_carla_tsum
  float step_size, sbc2, eps;
  float b1, omb1, b2, omb2, wd;  // (float)beta, (float)(1.0 - beta), (float)weight_decay
};

__device__ __forceinline__ void carla_adam_opt_one(const CarlaAdamOptArgs& a, float coef, float g, float& p, float& m,
                                                   float& v) {
  // One rounding per operation, in the order of include/ppo_carla.h: no contraction into fused multiply-adds,
  // so m and v equal an fp32 restatement of Adam::step bit for bit. k_carla_adam compiles the same way for
  // m and v (its literal betas make every product a plain multiply) and fuses only the parameter step's
  // multiply into its subtraction.
#pragma clang fp contract(off)
  float gv = g * coef;
  gv = gv + a.wd * p;
  m = m * a.b1 + gv * a.omb1;
  v = v * a.b2 + gv * gv * a.omb2;
  p = p - a.step_size * (m / (sqrtf(v) / a.sbc2 + a.eps));
}

// An element-wise stream: thread i < nvec owns the float4 group at begin + head + 4 i (16-byte aligned:
// every array is a hipMalloc base plus the same offset), the threads after them one element each of the
// head and of the tail. Plain loads and stores, every element written by exactly one thread.
__global__ __launch_bounds__(256) void k_carla_adam_opt(CarlaAdamOptArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const float coef = a.clip[1];
  if (i < a.nvec) {
    const long p = a.begin + a.head + 4 * i;
    const float4 g4 = *reinterpret_cast<const float4*>(a.G + p);
    float4 p4 = *reinterpret_cast<const float4*>(a.P + p);
    float4 m4 = *reinterpret_cast<const float4*>(a.m + p);
    float4 v4 = *reinterpret_cast<const float4*>(a.v + p);
    carla_adam_opt_one(a, coef, g4.x, p4.x, m4.x, v4.x);
    carla_adam_opt_one(a, coef, g4.y, p4.y, m4.y, v4.y);
    carla_adam_opt_one(a, coef, g4.z, p4.z, m4.z, v4.z);
    carla_adam_opt_one(a, coef, g4.w, p4.w, m4.w, v4.w);
    *reinterpret_cast<float4*>(a.m + p) = m4;
    *reinterpret_cast<float4*>(a.v + p) = v4;
    *reinterpret_cast<float4*>(a.P + p) = p4;
    return;
  }
  long k = i - a.nvec;  // the k-th scalar element: the head first, then the tail
  if (k >= a.n - 4 * a.nvec) return;
  if (k >= a.head) k += 4 * a.nvec;
  const long p = a.begin + k;
  float pv = a.P[p], mv = a.m[p], vv = a.v[p];
  carla_adam_opt_one(a, coef, a.G[p], pv, mv, vv);
  a.m[p] = mv;
  a.v[p] = vv;
  a.P[p] = pv;
}

}  // namespace

// the largest wgrad partial buffer any layer needs at max_batch rows
static size_t carla_part_floats(const ppo_carla_layout2& L, const CarlaNet& net, long B) {
  size_t m = 0;
  auto need = [&](int OC, int Kt, long Q) {
    const size_t f = plan_wgrad(OC, Kt, Q).part_floats;
    if (f > m) m = f;
  };
  for (int i = 0; i < PPO_CARLA_NCONV; ++i)
    need(L.conv_oc[i], carla_in_c(L, i) * L.conv_k[i] * L.conv_k[i], B * L.conv_oh[i] * L.conv_ow[i]);
  for (const CarlaLayer& e : net.layer) need(e.OUT, e.IN, B);
  need(L.A, 256, B);  // dist_mu, dist_sigma
  return m;
}

// c->small: where the per-tensor norm slices start (after the int64 tensor table at float 128)
constexpr int kSmallNorm = 128 + 4 * PPO_CARLA_MAX_TENSORS2;

static int carla_train_init(ppo_carla_t* c) {
  if (c->train_ready) return 0;
  const ppo_carla_layout2& L = c->L;
  const size_t B = (size_t)c->cfg.max_batch;
  int rc = 0;
  rc |= carla_alloc(&c->G, L.P);
  rc |= carla_alloc(&c->m, L.P);
  rc |= carla_alloc(&c->v, L.P);
  for (int i = 0; i < PPO_CARLA_NCONV - 1; ++i)
    rc |= carla_alloc(&c->dact[i], B * L.conv_oc[i] * L.conv_oh[i] * L.conv_ow[i]);
  for (int x = kBufS1; x < kBufCount; ++x)
    if (x != kBufState) rc |= carla_alloc(&c->d[x], B * carla_grad_stride(x));
  rc |= carla_alloc(&c->dhead, B * 2 * L.A);
  rc |= carla_alloc(&c->lp, B);
  rc |= carla_alloc(&c->ent, B);
  rc |= carla_alloc(&c->rowstat, B * 8);
  c->part_floats = carla_part_floats(L, c->net, (long)B);
  rc |= carla_alloc(&c->part, c->part_floats);
  size_t dcol_f = 1, wt_f = 1, zb_f = 1;
  for (int i = 1; i < PPO_CARLA_NCONV; ++i)
    if (dgrad_col_layer(L.conv_oh[i], L.conv_ow[i], L.conv_k[i], L.conv_s[i])) {
      const size_t kt = (size_t)L.conv_ic[i] * L.conv_k[i] * L.conv_k[i];
      dcol_f = std::max(dcol_f, B * kt * L.conv_oh[i] * L.conv_ow[i]);
      wt_f = std::max(wt_f, kt * L.conv_oc[i]);
      zb_f = std::max(zb_f, kt);
    }
  rc |= carla_alloc(&c->dcol, dcol_f);
  rc |= carla_alloc(&c->wt, wt_f);
  rc |= carla_alloc(&c->zbias, zb_f);
  if (c->any_ln) {
    size_t f = 1;
    for (const auto& l : c->ln)
      if (l.F) f = std::max(f, ln_part_floats((int)B, l.F));
    c->lnpart_floats = f;
    rc |= carla_alloc(&c->lnpart, f);
  }
  if (carla_pos(L)) {
    c->pospart_floats = pos_part_floats((int)B, L.conv_oc[0], L.conv_oh[0], L.conv_ow[0]);
    rc |= carla_alloc(&c->pospart, c->pospart_floats);
  }
  // [0,2) adv mean/std, [64,71) stats + {total, coef}, [128,384) int64 tensor table, [384,...) norm slices
  rc |= carla_alloc(&c->small, kSmallNorm + PPO_CARLA_MAX_TENSORS2 * kNormSplit);
  if (rc) return ppo_fail("ppo_carla_update: device allocation failed", -2);
  // tensor table (offsets / lengths as int64) after the scalars
  std::vector<long> tab(2 * PPO_CARLA_MAX_TENSORS2, 0);
  for (int t = 0; t < L.ntensors; ++t) {
    tab[t] = L.t_off[t];
    tab[PPO_CARLA_MAX_TENSORS2 + t] = L.t_grad[t] ? L.t_len[t] : 0;
  }
  if (hipMemcpy(c->small + 128, tab.data(), tab.size() * sizeof(long), hipMemcpyHostToDevice) != hipSuccess)
    return ppo_fail("ppo_carla_update: copy failed", -2);
  c->train_ready = true;
  return 0;
}

extern "C" int ppo_carla_update(ppo_carla_t* c, const ppo_carla_train_config* tc, int n, const uint8_t* bev,
                                const float* meas, const float* vmeas, const float* actions, const float* old_logp,
                                const float* adv, const float* ret, const float* old_v, float lr,
                                ppo_carla_update_stats* stats, void* stream) {
  if (!c || !tc || !bev || !meas || !actions || !old_logp || !adv || !ret || !old_v || (!vmeas && c->L.NV > 0))
    return ppo_fail("ppo_carla_update: null argument", -1);
  if (n <= 1 && tc->norm_adv) return ppo_fail("ppo_carla_update: advantage normalisation needs n >= 2", -1);
  if (n <= 0 || n > c->cfg.max_batch) return ppo_fail("ppo_carla_update: n must be in [1, max_batch]", -1);
  if (hipSetDevice(c->device) != hipSuccess) return ppo_fail("ppo_carla_update: hipSetDevice failed", -2);
  int rc = carla_train_init(c);
  if (rc) return rc;
  const ppo_carla_layout2& L = c->L;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  // forward with the given actions (ac_ppo_carla.cpp:543-546); activations stay in the context
  rc = ppo_carla_forward(c, n, bev, meas, vmeas, PPO_CARLA_GIVEN, actions, 0, 0, nullptr, c->lp, c->ent, nullptr,
                         nullptr, nullptr, s);
  if (rc) return rc;
  float* P = c->P;
  float* G = c->G;
  float* sm = c->small;
  if (tc->norm_adv) {
    if (c->comm) {  // ac_ppo_carla.cpp:564-578: averaged mean, summed squares, Bessel over world * n
      hipLaunchKernelGGL(k_carla_adv_part, dim3(1), dim3(256), 0, s, adv, n, sm, 0);
      if (ncclAllReduce(sm, sm, 1, ncclFloat, ncclAvg, c->comm, s) != ncclSuccess)
        return ppo_fail("ppo_carla_update: advantage mean all-reduce failed", -3);
      hipLaunchKernelGGL(k_carla_adv_part, dim3(1), dim3(256), 0, s, adv, n, sm, 1);
      if (ncclAllReduce(sm + 2, sm + 2, 1, ncclFloat, ncclSum, c->comm, s) != ncclSuccess)
        return ppo_fail("ppo_carla_update: advantage variance all-reduce failed", -3);
      hipLaunchKernelGGL(k_carla_adv_fin, dim3(1), dim3(64), 0, s, sm, (float)(c->world * n - 1));
    } else {
      hipLaunchKernelGGL(k_carla_advstats, dim3(1), dim3(256), 0, s, adv, n, sm);
    }
  }
  HeadBwdArgs hb{P,      L.hi,    L.lo,      c->hpre,   actions,     c->lp,        c->ent,        c->val,
                 old_logp, adv,   ret,       old_v,     sm,          n,            L.A,           c->cfg.beta_min,
                 tc->clip_coef, tc->ent_coef, tc->vf_coef, tc->norm_adv, tc->clip_vloss, c->dhead, c->d[kBufVal], c->rowstat};
  hipLaunchKernelGGL(k_carla_head_bwd, dim3((n + 63) / 64), dim3(64), 0, s, hb);
  int bad = 0;
  // y = x W^T + b on rows: dz [n][OUT] (stride dzs), x [n][IN] (stride xs)
  auto lin_w = [&](const float* dz, long dzs, int OUT, const float* x, long xs, int IN, long w, long b) {
    WgradArgs a{dz, dzs, OUT, 1, 1, x, nullptr, xs, IN, 1, 1, 1, 1, n, IN, 0, nullptr, c->wgrad_group};
    bad |= launch_wgrad(a, G + w, G + b, c->part, c->part_floats, s);
  };
  auto lin_d = [&](const float* dz, long dzs, int OUT, long w, int w_in, const float* x, long xs, float* dx, long dxs,
                   int IN, int accumulate) {
    DgradArgs a{dz, dzs, P + w, w_in, x, xs, dx, dxs, IN, 1, 1, OUT, 1, 1, 1, 1, n, accumulate};
    bad |= launch_dgrad(a, s);
  };
  // a normalised layer's backward, in place on its output gradient d (= dy * [y > 0] from the consuming
  // layers' lin_d / dgrad): dgamma / dbeta, then d = dz, which the layer's own wgrad / dgrad read
  auto ln_b = [&](int k, float* d, long ds) {
    const ppo_carla::Ln& l = c->ln[k];
    if (l.F)
      bad |= launch_ln_bwd(n, l.F, d, ds, l.z, l.F, P + l.g, l.stat, G + l.g, G + l.be, c->lnpart, c->lnpart_floats,
                           s);
  };
  const int A = L.A;
  // heads (carla_model.h:279-284): dist_mu / dist_sigma on the policy latent
  float* dp2 = c->d[kBufP2];
  lin_w(c->dhead, 2 * A, A, c->p2, 256, 256, L.mu_w, L.mu_b);
  lin_w(c->dhead + A, 2 * A, A, c->p2, 256, 256, L.sg_w, L.sg_b);
  lin_d(c->dhead, 2 * A, A, L.mu_w, 256, c->p2, 256, dp2, 256, 256, 0);
  lin_d(c->dhead + A, 2 * A, A, L.sg_w, 256, c->p2, 256, dp2, 256, 256, 1);
  // the Linear layers, last first: policy_head, value_head, linear, state_linear. A layer's input
  // gradient is stored, or added if a layer after it in the forward has stored it already (feat)
  bool written[kBufCount] = {};
  for (int i = kCarlaLayers - 1; i >= 0; --i) {
    const CarlaLayer& e = c->net.layer[i];
    float* dz = carla_grad(*c, e.out);
    const long dzs = carla_grad_stride(e.out);
    if (e.ln >= 0) ln_b(e.ln, dz, dzs);
    const float* x = e.in == kBufMeas ? meas : carla_buf(*c, e.in);
    lin_w(dz, dzs, e.OUT, x, e.in_stride, e.IN, e.w, e.b);
    if (e.in == kBufMeas) continue;  // the measurements get no gradient
    const long dxs = carla_grad_stride(e.in);
    // (of value_head.0's 256 + NV inputs only the 256 features get one)
    lin_d(dz, dzs, e.OUT, e.w, e.IN, x, e.in_stride, carla_grad(*c, e.in), dxs, (int)std::min<long>(e.IN, dxs),
          written[e.in]);
    written[e.in] = true;
  }
  // cnn (:236), last layer first; conv i reads act[i-1] (the image for i = 0)
  for (int i = PPO_CARLA_NCONV - 1; i >= 0; --i) {
    float* dz = i == PPO_CARLA_NCONV - 1 ? c->d[kBufEnc] : c->dact[i];
    const long dzs = i == PPO_CARLA_NCONV - 1 ? 1280 : (long)L.conv_oc[i] * L.conv_oh[i] * L.conv_ow[i];
    ln_b(ppo_carla::kLnConv + i, dz, dzs);
    const float* xf = i > 0 ? c->act[i - 1] : nullptr;
    bad |= launch_wgrad(wgrad_args(L, i, dz, dzs, xf, i ? nullptr : bev, n, c->wgrad_group), G + L.conv_w[i],
                        G + L.conv_b[i], c->part, c->part_floats, s, c->conv_img, c->c1bx, c->wgrad_t);
    if (i == 0 && carla_pos(L))  // the two coordinate planes' slices of cnn.0.weight's gradient
      bad |= launch_pos_wgrad(n, L.conv_oc[0], L.conv_oh[0], L.conv_ow[0], L.conv_k[0], L.conv_s[0], L.IH, L.IW, dz, dzs,
                              G + L.conv_w[0] + (long)L.C * L.conv_k[0] * L.conv_k[0],
                              (long)L.conv_ic[0] * L.conv_k[0] * L.conv_k[0], c->pospart, c->pospart_floats, s);
    if (i > 0) {
      const DgradArgs da = dgrad_args(L, i, P, dz, dzs, xf, c->dact[i - 1], n);
      if (c->dgrad_col && dgrad_col_layer(L.conv_oh[i], L.conv_ow[i], L.conv_k[i], L.conv_s[i]))
        bad |= launch_dgrad_col(da, c->wt, c->zbias, c->dcol, s);
      else
        bad |= launch_dgrad(da, s, c->conv_img, c->dgrad_q);
    }
  }
  if (bad) return ppo_fail("ppo_carla_update: no gradient kernel for this shape", -1);
  const long begin = 2;  // action_space_high / _low carry no gradient (registered with requires_grad false)
  // gradient average over ranks before clipping (ac_ppo_carla.cpp:608-616)
  if (c->comm && ncclAllReduce(G + begin, G + begin, (size_t)(L.P - begin), ncclFloat, ncclAvg, c->comm, s) != ncclSuccess)
    return ppo_fail("ppo_carla_update: gradient all-reduce failed", -3);
  // clip_grad_norm_ + Adam (ac_ppo_carla.cpp:618-619)
  const long* toff = (const long*)(sm + 128);
  hipLaunchKernelGGL(k_carla_tnorm, dim3(L.ntensors, kNormSplit), dim3(256), 0, s, G, toff,
                     toff + PPO_CARLA_MAX_TENSORS2, sm + kSmallNorm);
  hipLaunchKernelGGL(k_carla_tsum, dim3(1), dim3(64), 0, s, sm + kSmallNorm, L.ntensors, tc->max_grad_norm, sm + 70);
  c->step += 1;
  if (c->beta1 == 0.9 && c->beta2 == 0.999 && c->weight_decay == 0.0) {
    const double bc1 = 1.0 - std::pow(0.9, (double)c->step), bc2 = 1.0 - std::pow(0.999, (double)c->step);
    CarlaAdamArgs ad{P, G, c->m, c->v, begin, L.P - begin, sm + 70, (float)((double)lr / bc1), (float)std::sqrt(bc2),
                     tc->adam_eps};
    hipLaunchKernelGGL(k_carla_adam, dim3((unsigned)((L.P - begin + 255) / 256)), dim3(256), 0, s, ad);
  } else {  // ppo_carla_set_adam: the options as arguments (torch/optim/adam.cpp Adam::step)
    const double bc1 = 1.0 - std::pow(c->beta1, (double)c->step), bc2 = 1.0 - std::pow(c->beta2, (double)c->step);
    const long n = L.P - begin, head = std::min<long>((4 - begin % 4) % 4, n), nvec = (n - head) / 4;
    CarlaAdamOptArgs ad{P, G, c->m, c->v, begin, n, head, nvec, sm + 70, (float)((double)lr / bc1),
                        (float)std::sqrt(bc2), tc->adam_eps, (float)c->beta1, (float)(1.0 - c->beta1),
                        (float)c->beta2, (float)(1.0 - c->beta2), (float)c->weight_decay};
    const long threads = nvec + (n - 4 * nvec);
    hipLaunchKernelGGL(k_carla_adam_opt, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, ad);
  }
  hipLaunchKernelGGL(k_carla_stats, dim3(1), dim3(256), 0, s, c->rowstat, n, sm + 64);
  if (hipGetLastError() != hipSuccess) return ppo_fail("ppo_carla_update: launch failed", -2);
  if (int mrc = carla_params_mark(c, s)) return mrc;  // act lanes read the parameters after this step
  if (stats) {
    // loss statistics averaged over ranks (ac_ppo_carla.cpp:645-651); the total norm is global already
    if (c->comm && ncclAllReduce(sm + 64, sm + 64, 6, ncclFloat, ncclAvg, c->comm, s) != ncclSuccess)
      return ppo_fail("ppo_carla_update: statistics all-reduce failed", -3);
    float h[8];
    if (hipMemcpyAsync(h, sm + 64, sizeof h, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return ppo_fail("ppo_carla_update: stats copy failed", -2);
    stats->pg_loss = h[0];
    stats->v_loss = h[1];
    stats->entropy = h[2];
    stats->old_approx_kl = h[3];
    stats->approx_kl = h[4];
    stats->clipfrac = h[5];
    stats->grad_norm = h[6];
  }
  return 0;
}

static int carla_d2h(ppo_carla_t* c, const float* dev, float* host, long n, const char* what) {
  if (!c || !host) return ppo_fail(std::string(what) + ": null argument", -1);
  if (n != c->L.P) return ppo_fail(std::string(what) + ": expected " + std::to_string(c->L.P) + " floats", -1);
  if (!dev) return ppo_fail(std::string(what) + ": no training state yet (call ppo_carla_update first)", -1);
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess || hipMemcpy(host, dev, sizeof(float) * n, hipMemcpyDeviceToHost) != hipSuccess)
    return ppo_fail(std::string(what) + ": copy failed", -2);
  return 0;
}

extern "C" int ppo_carla_save_params(ppo_carla_t* c, float* host, long n) {
  return carla_d2h(c, c ? c->P : nullptr, host, n, "ppo_carla_save_params");
}

extern "C" int ppo_carla_last_grad(ppo_carla_t* c, float* host, long n) {
  return carla_d2h(c, c ? c->G : nullptr, host, n, "ppo_carla_last_grad");
}

extern "C" int ppo_carla_save_adam(ppo_carla_t* c, float* m_host, float* v_host, long n, long* step) {
  if (!c || !step) return ppo_fail("ppo_carla_save_adam: null argument", -1);
  if (!c->train_ready) {  // a fresh optimizer
    if (!m_host || !v_host || n != c->L.P) return ppo_fail("ppo_carla_save_adam: bad arguments", -1);
    std::fill(m_host, m_host + n, 0.0f);
    std::fill(v_host, v_host + n, 0.0f);
    *step = 0;
    return 0;
  }
  int rc = carla_d2h(c, c->m, m_host, n, "ppo_carla_save_adam");
  if (!rc) rc = carla_d2h(c, c->v, v_host, n, "ppo_carla_save_adam");
  *step = c->step;
  return rc;
}

extern "C" int ppo_carla_load_adam(ppo_carla_t* c, const float* m_host, const float* v_host, long n, long step) {
  if (!c || !m_host || !v_host) return ppo_fail("ppo_carla_load_adam: null argument", -1);
  if (n != c->L.P || step < 0) return ppo_fail("ppo_carla_load_adam: bad arguments", -1);
  if (hipSetDevice(c->device) != hipSuccess) return ppo_fail("ppo_carla_load_adam: hipSetDevice failed", -2);
  int rc = carla_train_init(c);
  if (rc) return rc;
  if (hipMemcpy(c->m, m_host, sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->v, v_host, sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess)
    return ppo_fail("ppo_carla_load_adam: copy failed", -2);
  c->step = step;
  return 0;
}

extern "C" int ppo_carla_set_adam(ppo_carla_t* c, double beta1, double beta2, double weight_decay) {
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
    return ppo_fail("ppo_carla_set_adam: beta1 and beta2 must be in [0, 1)", -1);
  if (!(weight_decay >= 0.0) || !std::isfinite(weight_decay))
    return ppo_fail("ppo_carla_set_adam: weight_decay must be finite and not negative", -1);
  if (!c) return ppo_fail("ppo_carla_set_adam: null argument", -1);
  c->beta1 = beta1;
  c->beta2 = beta2;
  c->weight_decay = weight_decay;
  return 0;
}

extern "C" int ppo_carla_get_adam(const ppo_carla_t* c, double* beta1, double* beta2, double* weight_decay) {
  if (!c || !beta1 || !beta2 || !weight_decay) return ppo_fail("ppo_carla_get_adam: null argument", -1);
  *beta1 = c->beta1;
  *beta2 = c->beta2;
  *weight_decay = c->weight_decay;
  return 0;
}

// test hook (ppo_carla.h): both Adam launches alone, timed with HIP events on the agent's stream
extern "C" int ppo_carla_debug_adam_time(ppo_carla_t* c, int reps, double beta1, double beta2, double weight_decay,
                                         float* us_default, float* us_opt) {
  if (!c || !us_default || !us_opt || reps <= 0) return ppo_fail("ppo_carla_debug_adam_time: bad argument", -1);
  if (hipSetDevice(c->device) != hipSuccess) return ppo_fail("ppo_carla_debug_adam_time: hipSetDevice failed", -2);
  if (int rc = carla_train_init(c)) return rc;
  const ppo_carla_layout2& L = c->L;
  hipStream_t s = c->stream;
  const float clip[2] = {0.0f, 1.0f};
  if (hipMemcpyAsync(c->small + 70, clip, sizeof clip, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return ppo_fail("ppo_carla_debug_adam_time: copy failed", -2);
  const long begin = 2, n = L.P - begin, head = std::min<long>((4 - begin % 4) % 4, n), nvec = (n - head) / 4;
  CarlaAdamArgs ad{c->P, c->G, c->m, c->v, begin, n, c->small + 70, 3e-4f, 1.0f, 1e-5f};
  CarlaAdamOptArgs ao{c->P, c->G, c->m, c->v, begin, n, head, nvec, c->small + 70, 3e-4f, 1.0f, 1e-5f,
                      (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)weight_decay};
  const unsigned gd = (unsigned)((n + 255) / 256), go = (unsigned)((nvec + (n - 4 * nvec) + 255) / 256);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
    return ppo_fail("ppo_carla_debug_adam_time: hipEventCreate failed", -2);
  float ms[2] = {0.0f, 0.0f};
  bool ok = true;
  for (int which = 0; which < 2 && ok; ++which) {
    for (int i = -3; i < reps; ++i) {  // three warm-up launches
      if (i == 0) ok = ok && hipEventRecord(e0, s) == hipSuccess;
      if (which == 0) hipLaunchKernelGGL(k_carla_adam, dim3(gd), dim3(256), 0, s, ad);
      else hipLaunchKernelGGL(k_carla_adam_opt, dim3(go), dim3(256), 0, s, ao);
    }
    ok = ok && hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
         hipEventElapsedTime(&ms[which], e0, e1) == hipSuccess && hipGetLastError() == hipSuccess;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (!ok) return ppo_fail("ppo_carla_debug_adam_time: timing failed", -2);
  *us_default = ms[0] * 1000.0f / (float)reps;
  *us_opt = ms[1] * 1000.0f / (float)reps;
  return carla_params_mark(c, s);
}

// ------------------------------------------------------------------------------------------
// data parallelism: RCCL communicator (replaces torchfort::Comm, distributed.cpp:81-224)
// ------------------------------------------------------------------------------------------
extern "C" int ppo_carla_comm_init(ppo_carla_t* c, const char* id, int rank, int world) {
  if (!c || !id) return ppo_fail("ppo_carla_comm_init: null argument", -1);
  if (world < 1 || rank < 0 || rank >= world) return ppo_fail("ppo_carla_comm_init: bad rank / world", -1);
  if (hipSetDevice(c->device) != hipSuccess) return ppo_fail("ppo_carla_comm_init: hipSetDevice failed", -2);
  if (c->comm) {
    (void)ncclCommDestroy(c->comm);
    c->comm = nullptr;
  }
  ncclUniqueId uid;
  static_assert(sizeof(ncclUniqueId) <= PPO_COMM_ID_BYTES, "ncclUniqueId size");
  memcpy(&uid, id, sizeof(uid));
  const ncclResult_t r = ncclCommInitRank(&c->comm, world, uid, rank);
  if (r != ncclSuccess) {
    c->comm = nullptr;
    return ppo_fail(std::string("ppo_carla_comm_init: ncclCommInitRank: ") + ncclGetErrorString(r), -3);
  }
  c->rank = rank;
  c->world = world;
  return 0;
}

extern "C" int ppo_carla_comm_broadcast_params(ppo_carla_t* c, int root) {
  if (!c) return ppo_fail("ppo_carla_comm_broadcast_params: null argument", -1);
  if (!c->comm) return 0;
  if (hipSetDevice(c->device) != hipSuccess) return ppo_fail("ppo_carla_comm_broadcast_params: hipSetDevice failed", -2);
  if (ncclBroadcast(c->P, c->P, (size_t)c->L.P, ncclFloat, root, c->comm, c->stream) != ncclSuccess)
    return ppo_fail("ppo_carla_comm_broadcast_params: ncclBroadcast failed", -3);
  if (int rc = carla_params_mark(c, c->stream)) return rc;
  return hipStreamSynchronize(c->stream) == hipSuccess ? 0 : ppo_fail("ppo_carla_comm_broadcast_params: sync failed", -2);
}

extern "C" int ppo_carla_comm_allreduce(ppo_carla_t* c, float* buf, long n, int average) {
  if (!c || !buf || n < 0) return ppo_fail("ppo_carla_comm_allreduce: bad argument", -1);
  if (!c->comm || n == 0) return 0;
  if (hipSetDevice(c->device) != hipSuccess) return ppo_fail("ppo_carla_comm_allreduce: hipSetDevice failed", -2);
  if (ncclAllReduce(buf, buf, (size_t)n, ncclFloat, average ? ncclAvg : ncclSum, c->comm, c->stream) != ncclSuccess)
    return ppo_fail("ppo_carla_comm_allreduce: ncclAllReduce failed", -3);
  return hipStreamSynchronize(c->stream) == hipSuccess ? 0 : ppo_fail("ppo_carla_comm_allreduce: sync failed", -2);
}

// ------------------------------------------------------------------------------------------
// internal entry points of the rollout object (ppo_carla_internal.hpp, ppo_carla_rollout.hip)
// ------------------------------------------------------------------------------------------
int carla_agent_info(const ppo_carla_t* c, CarlaAgentInfo* out) {
  if (!c || !out) return ppo_fail("carla_agent_info: null argument", -1);
  *out = CarlaAgentInfo{c->device, c->cfg.max_batch, c->stream};
  return 0;
}

int carla_params_mark(ppo_carla_t* c, hipStream_t s) {
  if (hipEventRecord(c->params_ev, s) != hipSuccess) return ppo_fail("carla_params_mark: hipEventRecord failed", -2);
  return 0;
}

int carla_params_wait(const ppo_carla_t* c, hipStream_t s) {
  if (hipStreamWaitEvent(s, c->params_ev, 0) != hipSuccess)
    return ppo_fail("carla_params_wait: hipStreamWaitEvent failed", -2);
  return 0;
}

int carla_stats_to_slot(ppo_carla_t* c, float* slot, hipStream_t s) {
  if (!c || !slot) return ppo_fail("carla_stats_to_slot: null argument", -1);
  if (!c->train_ready) return ppo_fail("carla_stats_to_slot: no update has run", -1);
  if (hipMemcpyAsync(slot, c->small + 64, kCarlaStatSlot * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
    return ppo_fail("carla_stats_to_slot: copy failed", -2);
  return 0;
}
