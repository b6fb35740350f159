/*
 * ppo_carla.h — the CaRL CNN agent's forward pass behind the same C-ABI
 * conventions as ppo_hip.h: int status (0 = OK), ppo_last_error() for the message, device
 * pointers for every array, the handle owns its device memory.
 *
 * Reference: include/carla/carla_model.h:21-318 (AgentImpl), with the defaults of
 * include/carla/carla_config.h: image_encoder "roach" (:71), use_layer_norm false (:78),
 * use_positional_encoding false (:117), obs_num_channels 15 (:58), bev 192 x 192 (:101-102),
 * obs_num_measurements 8 (:90), num_value_measurements 3 (:103), beta_min_a_b_value 1.0 (:56).
 *
 *   bev uint8 [N, C, 192, 192] / 255            (not divided under use_positional_encoding, below)
 *     -> cnn: Conv(C,8,5,s2) ReLU Conv(8,16,5,s2) ReLU Conv(16,32,5,s2) ReLU
 *             Conv(32,64,3,s2) ReLU Conv(64,128,3,s2) ReLU Conv(128,256,3,s1) ReLU   -> [N, 1024]
 *     state_linear: Linear(8,256) ReLU Linear(256,256) ReLU on measurements         -> [N, 256]
 *     linear: Linear(1024+256, 512) ReLU Linear(512, 256) ReLU                      -> features
 *   value_head: Linear(256+3, 256) ReLU Linear(256,256) ReLU Linear(256,1) on [features | vmeas]
 *   policy_head: Linear(256,256) ReLU Linear(256,256) ReLU; dist_mu / dist_sigma: Linear(256, A)
 *   alpha = softplus(mu) + beta_min, beta = softplus(sigma) + beta_min; Beta(alpha, beta)
 *   (rl_utils.h:87-132): sample | mean | roach_deterministic | given action (scaled to [0,1] and
 *   clamped to [1e-7, 1 + 1e-7], carla_model.h:251-260); log_prob and entropy summed over
 *   actions; the action is unscaled to [low, high] (:262-268).
 *
 * Parameter order = LibTorch named_parameters() of that module: action_space_high[],
 * action_space_low[] (no grad, own parameters first), then cnn.{0,2,4,6,8,10}.{weight,bias},
 * linear.{0,2}, state_linear.{0,2}, value_head.{0,2,4}, policy_head.{0,2}, dist_mu.0,
 * dist_sigma.0 (registration order, carla_model.h:108-192). Conv weights [OC, IC, k, k],
 * Linear weights [out, in].
 *
 * The reference's LayerNorm variants (image_encoder "roach_ln", :44-64: a LayerNorm over [C, H, W]
 * after every convolution; use_layer_norm, :113-175: a LayerNorm before every ReLU of the four MLPs,
 * the policy head's under use_layer_norm_policy_head) are a ppo_carla_arch given to
 * ppo_carla_create2; their tensors are described by ppo_carla_layout2 (cnn.{3i} / cnn.{3i+1},
 * linear.{0,1,3,4}, ..., value_head.{0,1,3,4,6}). Everything above — ppo_carla_layout,
 * ppo_carla_create(_ex), the default agent's kernels and results — is unchanged by them.
 * "roach_ln2" is not built.
 *
 * use_positional_encoding (:38-42, :222-236) is the pos_enc argument of ppo_carla_create3: cnn.0 takes
 * C + 2 channels, plane C = linspace(-1, 1, IH)[row], plane C + 1 = linspace(-1, 1, IW)[col]
 * (meshgrid "ij"). The two planes are never built: they are the same for every sample and constant along
 * one axis each, so their part of conv1's pre-activation is rowb[oc, oy] + colb[oc, ox], two small tables
 * computed from cnn.0.weight in every forward and added with the bias, and their weight gradient comes
 * from the row and column sums of conv1's pre-activation gradient (ppo_carla_pos.hip). A bev row stays
 * C * IH * IW bytes everywhere. THE BEV IS NOT NORMALISED WHEN THE SWITCH IS ON: the reference computes
 * bev / 255 and then overwrites it with concatenate({bev_semantics, grid0, grid1}, 1), whose first
 * operand is the raw uint8 tensor, promoted to fp32, so conv1 sees 0..255 and not 0..1. This is
 * reproduced as written: a checkpoint trained by the reference expects it. The inference server
 * (ppo_carla_inference) still refuses the switch; a positional checkpoint is served through
 * ppo_carla_forward, the Python binding, or the reference's own server (the .pth is LibTorch's).
 *
 * The training iteration around the agent (ac_ppo_carla.cpp:284-621) is a second handle,
 * ppo_carla_rollout_t, created from an agent: [T, E] storage of the dict observations on the device,
 * act-and-store, GAE over a full or preempted collection, the per-epoch permutation, the row gather of
 * each minibatch (k_carla_gather) and update_epochs x num_minibatches calls of ppo_carla_update without
 * a host synchronisation in between. See "rollout storage, GAE and the epoch loop" below for its three
 * rules: calls on one object are serial, every size is 64-bit, and a partial collection bootstraps
 * from the stored step. The agent's struct, kernels, defaults and results are unchanged by it.
 *
 * Concurrent collection (:355-417, one host thread, stream and batch-1 forward per env) is a third
 * handle, ppo_carla_lane_t, created from a rollout object: see "act lanes" below.
 */
#ifndef PPO_CARLA_H
#define PPO_CARLA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPO_CARLA_MAX_TENSORS 40
#define PPO_CARLA_NCONV 6

/* sample types: 0 "sample", 1 "mean", 2 given action, 3 "roach" (carla_model.h:287-303) */
enum { PPO_CARLA_SAMPLE = 0, PPO_CARLA_MEAN = 1, PPO_CARLA_GIVEN = 2, PPO_CARLA_ROACH = 3 };

typedef struct ppo_carla_layout {
  int C, IH, IW, NM, NV, A;
  long P;                       /* total floats */
  long hi, lo;                  /* action_space_high / low (no grad) */
  long conv_w[PPO_CARLA_NCONV], conv_b[PPO_CARLA_NCONV];
  int conv_ic[PPO_CARLA_NCONV], conv_oc[PPO_CARLA_NCONV], conv_k[PPO_CARLA_NCONV], conv_s[PPO_CARLA_NCONV];
  int conv_ih[PPO_CARLA_NCONV], conv_iw[PPO_CARLA_NCONV], conv_oh[PPO_CARLA_NCONV], conv_ow[PPO_CARLA_NCONV];
  long lin_w[2], lin_b[2];      /* linear.0: Linear(1024 + 256, 512), linear.2: Linear(512, 256) */
  long st_w[2], st_b[2];        /* state_linear.0: Linear(NM, 256), state_linear.2: Linear(256, 256) */
  long v_w[3], v_b[3];          /* value_head.{0,2,4}: Linear(256 + NV, 256), Linear(256, 256), Linear(256, 1) */
  long pi_w[2], pi_b[2];        /* policy_head.{0,2}: Linear(256, 256) x 2 */
  long mu_w, mu_b, sg_w, sg_b;  /* dist_mu.0, dist_sigma.0: Linear(256, A) */
  int ntensors;
  long t_off[PPO_CARLA_MAX_TENSORS];
  long t_len[PPO_CARLA_MAX_TENSORS];
  int t_grad[PPO_CARLA_MAX_TENSORS];
} ppo_carla_layout;

static inline long ppo_carla__add(ppo_carla_layout* L, long* cur, long n, int grad) {
  const long off = *cur;
  L->t_off[L->ntensors] = off;
  L->t_len[L->ntensors] = n;
  L->t_grad[L->ntensors] = grad;
  L->ntensors++;
  *cur += n;
  return off;
}

/* Returns 0, or -1 if the shapes do not give the reference's fixed n_flatten = 256 * 2 * 2
 * (carla_model.h:110) or are non-positive. */
static inline int ppo_carla_layout_init(ppo_carla_layout* L, int C, int IH, int IW, int NM, int NV, int A) {
  static const int oc[PPO_CARLA_NCONV] = {8, 16, 32, 64, 128, 256};
  static const int ks[PPO_CARLA_NCONV] = {5, 5, 5, 3, 3, 3};
  static const int st[PPO_CARLA_NCONV] = {2, 2, 2, 2, 2, 1};
  long cur = 0;
  int i, h = IH, w = IW, ic = C;
  if (C <= 0 || IH <= 0 || IW <= 0 || NM <= 0 || NV < 0 || A <= 0) return -1;
  L->C = C; L->IH = IH; L->IW = IW; L->NM = NM; L->NV = NV; L->A = A;
  L->ntensors = 0;
  L->hi = ppo_carla__add(L, &cur, 1, 0);
  L->lo = ppo_carla__add(L, &cur, 1, 0);
  for (i = 0; i < PPO_CARLA_NCONV; ++i) {
    L->conv_ic[i] = ic; L->conv_oc[i] = oc[i]; L->conv_k[i] = ks[i]; L->conv_s[i] = st[i];
    L->conv_ih[i] = h; L->conv_iw[i] = w;
    if (h < ks[i] || w < ks[i]) return -1;
    h = (h - ks[i]) / st[i] + 1;
    w = (w - ks[i]) / st[i] + 1;
    L->conv_oh[i] = h; L->conv_ow[i] = w;
    L->conv_w[i] = ppo_carla__add(L, &cur, (long)oc[i] * ic * ks[i] * ks[i], 1);
    L->conv_b[i] = ppo_carla__add(L, &cur, oc[i], 1);
    ic = oc[i];
  }
  if (256L * h * w != 1024) return -1;
  L->lin_w[0] = ppo_carla__add(L, &cur, 512L * (1024 + 256), 1); L->lin_b[0] = ppo_carla__add(L, &cur, 512, 1);
  L->lin_w[1] = ppo_carla__add(L, &cur, 256L * 512, 1);          L->lin_b[1] = ppo_carla__add(L, &cur, 256, 1);
  L->st_w[0] = ppo_carla__add(L, &cur, 256L * NM, 1);            L->st_b[0] = ppo_carla__add(L, &cur, 256, 1);
  L->st_w[1] = ppo_carla__add(L, &cur, 256L * 256, 1);           L->st_b[1] = ppo_carla__add(L, &cur, 256, 1);
  L->v_w[0] = ppo_carla__add(L, &cur, 256L * (256 + NV), 1);     L->v_b[0] = ppo_carla__add(L, &cur, 256, 1);
  L->v_w[1] = ppo_carla__add(L, &cur, 256L * 256, 1);            L->v_b[1] = ppo_carla__add(L, &cur, 256, 1);
  L->v_w[2] = ppo_carla__add(L, &cur, 256, 1);                   L->v_b[2] = ppo_carla__add(L, &cur, 1, 1);
  L->pi_w[0] = ppo_carla__add(L, &cur, 256L * 256, 1);           L->pi_b[0] = ppo_carla__add(L, &cur, 256, 1);
  L->pi_w[1] = ppo_carla__add(L, &cur, 256L * 256, 1);           L->pi_b[1] = ppo_carla__add(L, &cur, 256, 1);
  L->mu_w = ppo_carla__add(L, &cur, 256L * A, 1);                L->mu_b = ppo_carla__add(L, &cur, A, 1);
  L->sg_w = ppo_carla__add(L, &cur, 256L * A, 1);                L->sg_b = ppo_carla__add(L, &cur, A, 1);
  L->P = cur;
  return 0;
}

/* ---- LayerNorm variants (carla_model.h:44-64 image_encoder "roach_ln", :113-175 use_layer_norm) ----
 * All zero is the agent above. encoder_ln: a LayerNorm over [C, H, W] after every convolution
 * (cnn.{3i} conv, cnn.{3i+1} LayerNorm, cnn.{3i+2} ReLU); mlp_ln: a LayerNorm before every ReLU of
 * linear, state_linear and value_head (Linear at 0 / 3 / 6, LayerNorm at 1 / 4); policy_ln
 * (use_layer_norm_policy_head, read only when mlp_ln is set): the same for policy_head.
 * nn::LayerNorm defaults: biased variance, eps 1e-5, elementwise affine weight / bias of the
 * normalised shape. */
typedef struct ppo_carla_arch { int encoder_ln; int mlp_ln; int policy_ln; } ppo_carla_arch;

#define PPO_CARLA_MAX_TENSORS2 64

/* ppo_carla_layout plus the offsets of the LayerNorm weight (gamma) / bias (beta) tensors (-1 where
 * the arch has none). t_off / t_len / t_grad stay in named_parameters() order. */
typedef struct ppo_carla_layout2 {
  int C, IH, IW, NM, NV, A;
  long P;
  long hi, lo;
  long conv_w[PPO_CARLA_NCONV], conv_b[PPO_CARLA_NCONV];
  int conv_ic[PPO_CARLA_NCONV], conv_oc[PPO_CARLA_NCONV], conv_k[PPO_CARLA_NCONV], conv_s[PPO_CARLA_NCONV];
  int conv_ih[PPO_CARLA_NCONV], conv_iw[PPO_CARLA_NCONV], conv_oh[PPO_CARLA_NCONV], conv_ow[PPO_CARLA_NCONV];
  long lin_w[2], lin_b[2];
  long st_w[2], st_b[2];
  long v_w[3], v_b[3];
  long pi_w[2], pi_b[2];
  long mu_w, mu_b, sg_w, sg_b;
  ppo_carla_arch arch;          /* policy_ln normalised to 0 when mlp_ln is 0 */
  long conv_g[PPO_CARLA_NCONV], conv_be[PPO_CARLA_NCONV];  /* cnn.{3i+1}: [OC, OH, OW] */
  long lin_g[2], lin_be[2];     /* linear.{1,4}: [512], [256] */
  long st_g[2], st_be[2];       /* state_linear.{1,4}: [256] */
  long v_g[2], v_be[2];         /* value_head.{1,4}: [256] */
  long pi_g[2], pi_be[2];       /* policy_head.{1,4}: [256] */
  int ntensors;
  long t_off[PPO_CARLA_MAX_TENSORS2];
  long t_len[PPO_CARLA_MAX_TENSORS2];
  int t_grad[PPO_CARLA_MAX_TENSORS2];
} ppo_carla_layout2;

static inline long ppo_carla__add2(ppo_carla_layout2* L, long* cur, long n, int grad) {
  const long off = *cur;
  L->t_off[L->ntensors] = off;
  L->t_len[L->ntensors] = n;
  L->t_grad[L->ntensors] = grad;
  L->ntensors++;
  *cur += n;
  return off;
}

/* Returns 0; -1 as ppo_carla_layout_init; -2 if arch->encoder_ln is set with a bev other than
 * 192 x 192 (the reference hard-codes roach_ln's LayerNorm shapes, carla_model.h:45-62); -3 for a
 * pos_enc other than 0 or 1. arch NULL = all zero.
 *
 * pos_enc = 1 is use_positional_encoding (carla_model.h:38-42): cnn.0 is built with C + 2 input
 * channels, so conv_ic[0] == C + 2, cnn.0.weight is [8, C + 2, 5, 5] and every later offset moves by
 * 8 * 2 * 25 = 400. C stays the image's channel count; conv_ic[0] - C (0 or 2) IS the switch, no other
 * field records it. No tensor is added or renamed. */
static inline int ppo_carla_layout2_init_pos(ppo_carla_layout2* L, int C, int IH, int IW, int NM, int NV, int A,
                                             const ppo_carla_arch* arch, int pos_enc) {
  static const int oc[PPO_CARLA_NCONV] = {8, 16, 32, 64, 128, 256};
  static const int ks[PPO_CARLA_NCONV] = {5, 5, 5, 3, 3, 3};
  static const int st[PPO_CARLA_NCONV] = {2, 2, 2, 2, 2, 1};
  long cur = 0;
  int i, h = IH, w = IW, ic = C + (pos_enc ? 2 : 0);
  const int eln = arch && arch->encoder_ln, mln = arch && arch->mlp_ln, pln = mln && arch->policy_ln;
  if (pos_enc != 0 && pos_enc != 1) return -3;
  if (C <= 0 || IH <= 0 || IW <= 0 || NM <= 0 || NV < 0 || A <= 0) return -1;
  if (eln && (IH != 192 || IW != 192)) return -2;
  L->C = C; L->IH = IH; L->IW = IW; L->NM = NM; L->NV = NV; L->A = A;
  L->arch.encoder_ln = eln; L->arch.mlp_ln = mln; L->arch.policy_ln = pln;
  L->ntensors = 0;
  L->hi = ppo_carla__add2(L, &cur, 1, 0);
  L->lo = ppo_carla__add2(L, &cur, 1, 0);
  for (i = 0; i < PPO_CARLA_NCONV; ++i) {
    L->conv_ic[i] = ic; L->conv_oc[i] = oc[i]; L->conv_k[i] = ks[i]; L->conv_s[i] = st[i];
    L->conv_ih[i] = h; L->conv_iw[i] = w;
    if (h < ks[i] || w < ks[i]) return -1;
    h = (h - ks[i]) / st[i] + 1;
    w = (w - ks[i]) / st[i] + 1;
    L->conv_oh[i] = h; L->conv_ow[i] = w;
    L->conv_w[i] = ppo_carla__add2(L, &cur, (long)oc[i] * ic * ks[i] * ks[i], 1);
    L->conv_b[i] = ppo_carla__add2(L, &cur, oc[i], 1);
    L->conv_g[i] = eln ? ppo_carla__add2(L, &cur, (long)oc[i] * h * w, 1) : -1;
    L->conv_be[i] = eln ? ppo_carla__add2(L, &cur, (long)oc[i] * h * w, 1) : -1;
    ic = oc[i];
  }
  if (256L * h * w != 1024) return -1;
#define PPO_CARLA__LIN(W, B, G, BE, k, nw, nb, ln)                                   \
  L->W[k] = ppo_carla__add2(L, &cur, (nw), 1); L->B[k] = ppo_carla__add2(L, &cur, (nb), 1); \
  L->G[k] = (ln) ? ppo_carla__add2(L, &cur, (nb), 1) : -1; L->BE[k] = (ln) ? ppo_carla__add2(L, &cur, (nb), 1) : -1
  PPO_CARLA__LIN(lin_w, lin_b, lin_g, lin_be, 0, 512L * (1024 + 256), 512, mln);
  PPO_CARLA__LIN(lin_w, lin_b, lin_g, lin_be, 1, 256L * 512, 256, mln);
  PPO_CARLA__LIN(st_w, st_b, st_g, st_be, 0, 256L * NM, 256, mln);
  PPO_CARLA__LIN(st_w, st_b, st_g, st_be, 1, 256L * 256, 256, mln);
  PPO_CARLA__LIN(v_w, v_b, v_g, v_be, 0, 256L * (256 + NV), 256, mln);
  PPO_CARLA__LIN(v_w, v_b, v_g, v_be, 1, 256L * 256, 256, mln);
  L->v_w[2] = ppo_carla__add2(L, &cur, 256, 1); L->v_b[2] = ppo_carla__add2(L, &cur, 1, 1);
  PPO_CARLA__LIN(pi_w, pi_b, pi_g, pi_be, 0, 256L * 256, 256, pln);
  PPO_CARLA__LIN(pi_w, pi_b, pi_g, pi_be, 1, 256L * 256, 256, pln);
#undef PPO_CARLA__LIN
  L->mu_w = ppo_carla__add2(L, &cur, 256L * A, 1); L->mu_b = ppo_carla__add2(L, &cur, A, 1);
  L->sg_w = ppo_carla__add2(L, &cur, 256L * A, 1); L->sg_b = ppo_carla__add2(L, &cur, A, 1);
  L->P = cur;
  return 0;
}

static inline int ppo_carla_layout2_init(ppo_carla_layout2* L, int C, int IH, int IW, int NM, int NV, int A,
                                         const ppo_carla_arch* arch) {
  /* not "return f(...)": tests/test_capi_cpu.py reads a line of that form as the declaration of an export */
  const int rc = ppo_carla_layout2_init_pos(L, C, IH, IW, NM, NV, A, arch, 0);
  return rc;
}

/* the exported form of ppo_carla_layout2_init (bindings); the message names the reason */
int ppo_carla_layout2_fill(ppo_carla_layout2* L, int C, int IH, int IW, int NM, int NV, int A,
                           const ppo_carla_arch* arch);
/* the exported form of ppo_carla_layout2_init_pos; pos_enc = 0 fills what ppo_carla_layout2_fill fills */
int ppo_carla_layout2_fill_pos(ppo_carla_layout2* L, int C, int IH, int IW, int NM, int NV, int A,
                               const ppo_carla_arch* arch, int pos_enc);
/* named_parameters() name of tensor t ("cnn.1.weight", ...) into buf (NUL-terminated, truncated to
 * len); returns 0, -1 for a bad index or buffer */
int ppo_carla_tensor_name(const ppo_carla_layout2* L, int t, char* buf, int len);

typedef struct ppo_carla_config {
  int obs_channels;            /* 15 */
  int bev_h, bev_w;            /* 192, 192 */
  int num_measurements;        /* 8 */
  int num_value_measurements;  /* 3 */
  int action_dim;              /* 2 (steer, acceleration) */
  float beta_min;              /* 1.0 */
  int max_batch;               /* largest n passed to ppo_carla_forward */
  uint64_t seed;               /* Philox sampling key (same contract as ppo_hip.h) */
  int rank;
} ppo_carla_config;

typedef struct ppo_carla ppo_carla_t;

/* carla_model.h:35-206 (the module) — allocates parameters and activation buffers on `device`. */
int ppo_carla_create(const ppo_carla_config* cfg, int device, ppo_carla_t** out);
/* options: NULL / "" (defaults) or "key=value" pairs separated by ',':
 *   conv1=packed|staged|generic  conv1 forward with packed taps (k_conv_img3, default), conv1 forward
 *                              and weight gradient with the image patch staged in LDS (staged; the
 *                              weight gradient's form for packed too), or the generic implicit-GEMM
 *                              kernels (A/B tests)
 *   conv1_mfma=auto|bx3|f32    the packed conv1 forward and the staged conv1 weight gradient with their
 *                              products as split-bf16 MFMAs (bx3, auto: the raw byte operand is exact
 *                              in bf16, the fp32 operand's three bf16 pieces make every product exact;
 *                              fp32 accumulation on 16x16x32 bf16 MFMAs) or on 16x16x4 fp32 MFMAs
 *   conv_fwd=tiled|generic     conv2 / conv3 forward from LDS-staged input patches (k_conv_t / k_conv_t2,
 *                              default) or the generic gather kernel (A/B tests; another fp32 sum order)
 *   conv_wgrad=tiled|generic   conv2 / conv3 weight gradients from LDS-staged tiles (k_wgrad_t / k_wgrad_t2,
 *                              default) or the generic k_wgrad
 *   conv_dgrad=quad|staged     conv2 / conv3 input gradients with the four stride-2 parity classes of a
 *                              quad sharing one dZ operand (k_dgrad_q / k_dgrad_q2, default) or
 *                              k_dgrad_s2 / k_dgrad (needs conv1=staged|packed)
 *   deep_dgrad=col|gather      conv6's input gradient as a dense GEMM into columns + col2im (default) or
 *                              k_dgrad
 *   tail=staged|fused|layers   forwards of n <= 64 rows: the MLP tail after the CNN as one launch per
 *                              dependency stage (default), one cooperative launch with a grid barrier
 *                              between stages, or one k_conv / k_conv_fin pair per layer (the path of
 *                              larger batches); bitwise equal
 *   wgrad_group_bytes=N        (tests) the generic fp32 weight-gradient kernel runs its samples in groups
 *                              whose input stays below N bytes, each group's sums added to the previous
 *                              ones'; without it the groups start at 0x70000000 bytes (the kernel's 32-bit
 *                              buffer offsets), so no batch size is refused */
int ppo_carla_create_ex(const ppo_carla_config* cfg, int device, const char* options, ppo_carla_t** out);
int ppo_carla_destroy(ppo_carla_t* c);
int ppo_carla_get_layout(const ppo_carla_t* c, ppo_carla_layout* out);
/* ppo_carla_create_ex with an architecture (arch NULL = all zero = ppo_carla_create_ex). Refused
 * before any HIP call: encoder_ln with a bev other than 192 x 192, and an explicit tail=fused or
 * tail=staged with any LayerNorm (such an agent always runs the per-layer forward, one k_carla_ln
 * after each normalised layer). roach_ln2 is not built; use_positional_encoding is ppo_carla_create3's.
 * ppo_carla_get_layout2 serves every agent (the default one's offsets are ppo_carla_layout's);
 * ppo_carla_get_layout fails on a LayerNorm agent and on a positional one, whose tensors it cannot
 * describe. */
int ppo_carla_create2(const ppo_carla_config* cfg, const ppo_carla_arch* arch, int device, const char* options,
                      ppo_carla_t** out);
/* ppo_carla_create2 with use_positional_encoding (pos_enc = 1; see the head of this file). pos_enc = 0 IS
 * ppo_carla_create2: the same kernels, launches and bits. cfg->obs_channels stays the image's channel
 * count; the layout says conv_ic[0] == obs_channels + 2. Every conv1= and conv1_mfma= option is carried:
 * each conv1 kernel reads the image channels of the wider filters, takes the image scale (1 instead of
 * 1 / 255) as an argument and adds the two tables in its epilogue. Refused before any HIP call, besides
 * what ppo_carla_create2 refuses: a pos_enc other than 0 or 1. */
int ppo_carla_create3(const ppo_carla_config* cfg, const ppo_carla_arch* arch, int pos_enc, int device,
                      const char* options, ppo_carla_t** out);
int ppo_carla_get_layout2(const ppo_carla_t* c, ppo_carla_layout2* out);
/* host floats in named_parameters() order (torch::load of a model_*.pth, ac_ppo_carla.cpp) */
int ppo_carla_load_params(ppo_carla_t* c, const float* host, long n);
/* AgentImpl::forward (carla_model.h:270-318) for n rows; every array is a device pointer:
 *   bev uint8 [n, C, IH, IW], meas [n, NM], vmeas [n, NV], action_in [n, A] (GIVEN only);
 *   outputs (any may be NULL): action [n, A] in [low, high], logprob [n], entropy [n],
 *   value [n], alpha [n, A], beta [n, A].
 * SAMPLE draws with the Philox contract of ppo_hip.h (env = env_base + row, step = step_id). */
int ppo_carla_forward(ppo_carla_t* c, int n, const uint8_t* bev, const float* meas, const float* vmeas,
                      int sample_type, const float* action_in, long env_base, long step_id, float* action,
                      float* logprob, float* entropy, float* value, float* alpha, float* beta, void* stream);

/* ---- training (ac_ppo_carla.cpp:529-620): one PPO minibatch step --------------------------------
 * Loss = pg_loss - ent_coef * entropy + vf_coef * v_loss exactly as the MLP agents (clipped
 * surrogate, clipped value loss, minibatch advantage normalisation with Bessel's correction),
 * backward through heads, MLPs and all six convolutions, clip_grad_norm_(max_grad_norm), Adam
 * (eps = adam_eps, bias-corrected; betas 0.9 / 0.999 and weight_decay 0 unless ppo_carla_set_adam
 * says otherwise), all on the device. */
typedef struct ppo_carla_train_config {
  float clip_coef;      /* 0.2 */
  float ent_coef;       /* 0.0 */
  float vf_coef;        /* 0.5 */
  float max_grad_norm;  /* 0.5 */
  float adam_eps;       /* 1e-5 */
  int norm_adv;         /* 1 */
  int clip_vloss;       /* 1 */
} ppo_carla_train_config;

typedef struct ppo_carla_update_stats {
  float pg_loss, v_loss, entropy, old_approx_kl, approx_kl, clipfrac;
  float grad_norm;  /* total norm before clipping */
} ppo_carla_update_stats;

/* One minibatch of n <= max_batch rows (device pointers): bev uint8 [n, C, IH, IW], meas [n, NM],
 * vmeas [n, NV], actions [n, A] (env space), old_logp / adv / ret / old_v [n]. stats may be NULL
 * (no host synchronisation then). */
int ppo_carla_update(ppo_carla_t* c, const ppo_carla_train_config* tc, int n, const uint8_t* bev, const float* meas,
                     const float* vmeas, const float* actions, const float* old_logp, const float* adv,
                     const float* ret, const float* old_v, float lr, ppo_carla_update_stats* stats, void* stream);
/* parameters (named_parameters() order) and the raw gradient of the last update, to host */
int ppo_carla_save_params(ppo_carla_t* c, float* host, long n);
int ppo_carla_last_grad(ppo_carla_t* c, float* host, long n);
/* Adam moments in the same flat order, and the step count */
int ppo_carla_save_adam(ppo_carla_t* c, float* m_host, float* v_host, long n, long* step);
int ppo_carla_load_adam(ppo_carla_t* c, const float* m_host, const float* v_host, long n, long step);
/* The optimizer's betas and weight decay (the reference's Adam(lr).eps(adam_eps).weight_decay(weight_decay)
 * .betas(beta_1, beta_2), ac_ppo_carla.cpp:246; defaults 0.9, 0.999, 0). They belong to the agent and
 * persist across ppo_carla_update, ppo_carla_rollout_train and ppo_carla_load_adam. LibTorch's C++
 * Adam::step after clip_grad_norm_, on every trainable tensor (LayerNorm weights and biases included;
 * action_space_high / _low are never touched):
 *   g = G * coef;  g += (float)wd * p            (coupled L2, not AdamW)
 *   m = m * (float)b1 + g * (float)(1.0 - b1);   v = v * (float)b2 + g * g * (float)(1.0 - b2)
 *   p -= step_size * m / (sqrt(v) / sqrt(bc2) + eps),  step_size = lr / bc1, bc = 1 - pow(b, step) in double
 * Options of exactly (0.9, 0.999, 0) launch k_carla_adam, which has them compiled in: such an agent's
 * bits are those of one that never called ppo_carla_set_adam. Any other options launch k_carla_adam_opt.
 * Refused before any HIP call: NULL arguments, a beta outside [0, 1), a negative or non-finite weight
 * decay. Like ppo_carla_load_adam, it must not be called while an update or a lane call of the agent is
 * inside the library. */
int ppo_carla_set_adam(ppo_carla_t* c, double beta1, double beta2, double weight_decay);
int ppo_carla_get_adam(const ppo_carla_t* c, double* beta1, double* beta2, double* weight_decay);

/* test hook: `reps` back-to-back launches of k_carla_adam, then of k_carla_adam_opt with the given options,
 * over the agent's trainable range, each run timed with HIP events on the agent's stream after three
 * warm-up launches; microseconds per launch. It steps the agent's parameters and moments with whatever
 * gradient is there (lr 3e-4, no bias correction) and leaves the step count and options alone: for a
 * scratch agent only. */
int ppo_carla_debug_adam_time(ppo_carla_t* c, int reps, double beta1, double beta2, double weight_decay,
                              float* us_default, float* us_opt);

/* ---- test hooks: the LayerNorm launches of the agent on caller arrays (device pointers) ----------
 * forward: y[r, 0..F) = relu(layer_norm(z[r, 0..F)) * gamma + beta) for n rows of strides in_stride /
 * out_stride, stat[r] = {mean, rstd} (k_carla_ln; k_carla_ln_big for rows of 4 096 floats and more).
 * backward: dz [n, F] (dense) from dy (dense [n, F]), the ReLU mask y > 0 and the forward's z / stat;
 * dgamma / dbeta [F]. The agent's own backward receives dy already masked by the consuming layer's
 * input-gradient kernel; the hook applies that mask with one extra launch, then runs the agent's
 * column pass (k_carla_ln_dgb + k_carla_ln_dgb_sum) and row pass (k_carla_ln_bwd). */
int ppo_carla_debug_ln_forward(int n, int F, const float* z, long in_stride, const float* gamma, const float* beta,
                               float* y, long out_stride, float* stat, void* stream);
int ppo_carla_debug_ln_backward(int n, int F, const float* z, long in_stride, const float* gamma, const float* stat,
                                const float* y, long out_stride, const float* dy, float* dz, float* dgamma,
                                float* dbeta, void* stream);

/* ---- test hooks: positional encoding (ppo_carla_pos.hip) ------------------------------------------
 * pos_grid: host[0..n) = the library's torch.linspace(-1, 1, n) in fp32 (host only, no HIP call).
 * pos_bias: the agent's table launch on caller arrays (device pointers): rowb [OC][OH], colb [OC][OW]
 * from W [OC][IC_total][K][K], whose planes C and C + 1 are the two coordinate planes' weights
 * (OH = (IH - K) / S + 1, OW likewise).
 * pos_wgrad: the agent's reduction (k_pos_rq) and finish (k_pos_wfin) on dz [n][OC][OH][OW] (dense,
 * device): dw_pos [OC][2][K][K], with partial-sum buffers sized for max_n >= n as an agent's are for
 * max_batch. Both synchronise the stream. */
int ppo_carla_debug_pos_grid(int n, float* host);
int ppo_carla_debug_pos_bias(int OC, int IC_total, int C, int K, int S, int IH, int IW, const float* W_dev,
                             float* rowb_dev, float* colb_dev, void* stream);
int ppo_carla_debug_pos_wgrad(int n, int max_n, int OC, int OH, int OW, int K, int S, int IH, int IW,
                              const float* dz_dev, float* dw_pos_dev, void* stream);

/* ---- data parallelism (ac_ppo_carla.cpp:243, 561-616; torchfort::Comm, distributed.cpp:81-224) ----
 * One RCCL communicator per agent; id from ppo_comm_unique_id (ppo_hip.h), PPO_COMM_ID_BYTES bytes.
 * With a communicator attached (any world >= 1), every ppo_carla_update
 *   - takes the minibatch advantage mean as the rank average of the local means and the std
 *     from the all-reduced sum of squares with Bessel's correction over world * n - 1
 *     (ac_ppo_carla.cpp:561-580),
 *   - all-reduces (average) the gradient of every trainable tensor before clip_grad_norm_ (:608-616),
 *   - averages the returned loss statistics over ranks (:645-651; grad_norm is already global).
 * world = 1 runs the same collective sequence over a one-rank communicator (results equal the
 * communicator-free update bit for bit). */
int ppo_carla_comm_init(ppo_carla_t* c, const char* id, int rank, int world);
/* ac_ppo_carla.cpp:241-244: every parameter from `root` to all ranks */
int ppo_carla_comm_broadcast_params(ppo_carla_t* c, int root);
/* in-place all-reduce (sum, or average) of buf[0..n) (device pointer) over the agent's communicator on
 * the agent's stream, then a stream synchronisation; no communicator: the identity (:439-441, :346) */
int ppo_carla_comm_allreduce(ppo_carla_t* c, float* buf, long n, int average);

/* ---- rollout storage, GAE and the epoch loop (ac_ppo_carla.cpp:284-621) -------------------------
 * A rollout object sits beside an agent and holds one collection of T steps x E envs on the agent's
 * device: bev uint8 [T, E, C, IH, IW], measurements [T, E, NM], value_measurements [T, E, NV],
 * actions [T, E, A] and logprobs / rewards / dones / values / advantages / returns [T, E], all fp32
 * but the bev (:285-295). It computes through ppo_carla_forward and ppo_carla_update only, so what
 * those document (sampling contract, loss, data parallelism of an attached communicator) holds here.
 *
 * Serial calls. The agent's activation buffers are shared by every forward and update, and the
 * object's minibatch staging buffers by every train call: calls on one rollout object, and on its
 * agent while the object is in use, must be made one after the other (from any one thread at a
 * time), each on the same stream (NULL = the agent's own). The per-thread concurrency of
 * ppo_rollout_act (one thread and stream per env range) is NOT offered by these calls: ranges of one
 * step are passed in successive calls. It is what act lanes are for (below: ppo_carla_lane_t, one host
 * thread, one stream and one private set of activation buffers per env). The agent must outlive the
 * object.
 *
 * 64-bit sizing. One bev row is C * IH * IW bytes (552 960 for 15 x 192 x 192): 7 767 rows pass
 * 2^32 bytes, and a collection of 65 536 rows is 36 GB. Every size, row offset and byte index of
 * the storage, the staging buffers and the gather kernel is a 64-bit integer; only the row
 * indices of a permutation are int32 (T * E < 2^31 is checked).
 *
 * Partial collections (DD-PPO preemption, :399-436, :490-504, :531-538). num_steps_collected < T
 * says that every env stored the steps [0, num_steps_collected) and, before it stopped, also
 * executed rollout_act for step num_steps_collected (the preemption test runs after the step, so
 * the stored values / dones of that step exist). GAE then bootstraps its last step from the STORED
 * step num_steps_collected — values[t + 1], dones[t + 1] whenever t != T - 1, the reference's
 * recurrence and what ppo_compute_gae documents — and the next observation's value is computed
 * but not read. Training permutes the Bc = num_steps_collected * E collected rows and repeats the
 * permutation up to the full batch B = T * E, truncated (b_inds.repeat(ceil(B / Bc))[:B]). */
typedef struct ppo_carla_rollout_config {
  int num_steps, num_envs;           /* T, E: envs on this device (num_envs_per_proc) */
  int update_epochs, num_minibatches;
  float gamma, gae_lambda;           /* 0.99, 0.95 */
  uint64_t seed;                     /* permutation key (seed, rank, epoch counter), as ppo_hip.h */
  int rank;
} ppo_carla_rollout_config;

typedef struct ppo_carla_rollout ppo_carla_rollout_t;

/* ppo_carla_rollout_buffer's `which` */
enum {
  PPO_CARLA_BUF_BEV = 0, PPO_CARLA_BUF_MEAS, PPO_CARLA_BUF_VMEAS, PPO_CARLA_BUF_ACTIONS, PPO_CARLA_BUF_LOGP,
  PPO_CARLA_BUF_REWARDS, PPO_CARLA_BUF_DONES, PPO_CARLA_BUF_VALUES, PPO_CARLA_BUF_ADV, PPO_CARLA_BUF_RETURNS,
  PPO_CARLA_BUF_NEXT_VALUE,          /* [E]: the bootstrap value of the last ppo_carla_rollout_gae */
  PPO_CARLA_BUF_COUNT
};

/* Refused before any HIP call: a NULL agent / config / out, non-positive sizes, T * E not divisible
 * by num_minibatches (or 2^31 and more), an agent whose max_batch is below
 * max(E, T * E / num_minibatches). The storage starts zeroed. */
int ppo_carla_rollout_create(ppo_carla_t* agent, const ppo_carla_rollout_config* cfg, ppo_carla_rollout_t** out);
int ppo_carla_rollout_destroy(ppo_carla_rollout_t* r);
/* :365-379 for envs [env_begin, env_end) at `step`: stores the observation rows and next_done, runs
 * ppo_carla_forward(SAMPLE, env_base = env_begin, step_id = iteration * T + step) on them and stores
 * action, log-prob and value; action_out [env_end - env_begin, A] (may be NULL) receives the actions.
 * Device pointers that address row env_begin: bev [n, C, IH, IW], meas [n, NM], vmeas [n, NV],
 * next_done [n]. */
int ppo_carla_rollout_act(ppo_carla_rollout_t* r, int step, int env_begin, int env_end, const uint8_t* bev,
                          const float* meas, const float* vmeas, const float* next_done, float* action_out,
                          void* stream);
/* :385: rewards[step, env_begin .. env_end) = reward[0 .. env_end - env_begin) (device pointer) */
int ppo_carla_rollout_reward(ppo_carla_rollout_t* r, int step, int env_begin, int env_end, const float* reward,
                             void* stream);
/* :484-504: the bootstrap value from one forward on the next observation [E, ...] (value output only),
 * advantages over steps [0, num_steps_collected), returns = advantages + values. */
int ppo_carla_rollout_gae(ppo_carla_rollout_t* r, const uint8_t* next_bev, const float* next_meas,
                          const float* next_vmeas, const float* next_done, int num_steps_collected, void* stream);
/* :531-621: update_epochs x num_minibatches optimizer steps on the agent's stream. Per epoch the
 * permutation of make_perm_key(seed, rank, iteration * update_epochs + epoch, Bc) over the collected
 * rows, repeated and truncated to B = T * E; perms_dev int32 [update_epochs][B] (device, may be NULL)
 * replaces it. Each minibatch's rows are gathered into contiguous staging buffers (k_carla_gather)
 * and passed to ppo_carla_update. `last` (may be NULL) receives the last minibatch's statistics,
 * rank-averaged as ppo_carla_update's; mean_clipfrac (may be NULL) the mean clipfrac over all
 * minibatches (:637, rank-averaged, :651). There is no host synchronisation between minibatches, and
 * none at all when both are NULL. Advances the iteration counter. */
int ppo_carla_rollout_train(ppo_carla_rollout_t* r, const ppo_carla_train_config* tc, float lr,
                            int num_steps_collected, const int32_t* perms_dev, ppo_carla_update_stats* last,
                            float* mean_clipfrac);
/* losses/discounted_returns (:626-658, :701): *out (host) = the mean of the returns of the last
 * ppo_carla_rollout_gae over the num_steps_collected * E collected rows, repeated and truncated to
 * B = T * E as the permutation is, then averaged over the ranks of an attached communicator. One
 * fixed-order reduction (k_carla_returns_mean, one block) on the agent's stream: two calls give the
 * same bits, and a one-rank communicator changes none. Synchronises that stream. Refused like
 * ppo_carla_rollout_train while a lane call is inside the library. */
int ppo_carla_rollout_returns_mean(ppo_carla_rollout_t* r, int num_steps_collected, float* out);
/* device pointer of a storage array (PPO_CARLA_BUF_*) */
int ppo_carla_rollout_buffer(ppo_carla_rollout_t* r, int which, void** dev_ptr);
/* host copy of the indices the last ppo_carla_rollout_train used: n = update_epochs * T * E */
int ppo_carla_rollout_last_perms(ppo_carla_rollout_t* r, int32_t* host, long n);
long ppo_carla_rollout_iteration(const ppo_carla_rollout_t* r);
int ppo_carla_rollout_set_iteration(ppo_carla_rollout_t* r, long iteration);

/* ---- act lanes: concurrent collection (ac_ppo_carla.cpp:355-417) -----------------------------------
 * The reference collects with one host thread, one stream and one batch-1 forward per env, so that E
 * simulators tick at the same time. A lane is that thread's handle: created from a rollout object, it
 * owns a stream, a private one-row copy of every buffer a forward writes (conv outputs, MLP
 * activations, split-K partials, the packed conv1 weight table, the LayerNorm z / stat buffers, the
 * cooperative tail's barrier counter) and a pinned host buffer for one observation and one action.
 * Parameters stay shared: collection only reads them.
 *
 * Threads. Lanes of one rollout object may be used from different threads at the same time; one lane is
 * used by one thread at a time. Every lane call selects the agent's device for the calling thread;
 * ppo_last_error is thread-local. Two lanes must not act for the same (step, env) of one collection.
 *
 * Ordering is kept by events, not by the caller: ppo_carla_rollout_gae and _train make their stream wait
 * for the last queued work of every lane (a ppo_carla_lane_reward still in flight included), and a
 * lane's next act waits for the last ppo_carla_rollout_gae / _train of its object and for the agent's
 * last ppo_carla_update, ppo_carla_load_params or ppo_carla_comm_broadcast_params.
 *
 * What stays forbidden: ppo_carla_update, ppo_carla_load_params, ppo_carla_comm_broadcast_params,
 * ppo_carla_rollout_gae / _train / _set_iteration / _destroy or the creation and destruction of lanes
 * while a lane call of that object is inside the library (join the collecting threads first; what a
 * returned call left queued is covered by the events). A lane call that finds such a call inside the
 * library, or the reverse, is refused where the library can tell (-1, "... while ..."): rollout_gae,
 * rollout_train, lane_create and lane_destroy check the object's count of lane calls in progress, and a
 * lane call checks that none of those four is in progress. The lanes must be destroyed before their
 * rollout object. */
#define PPO_CARLA_MAX_LANES 64

typedef struct ppo_carla_lane ppo_carla_lane_t;

/* Refused before any HIP call: NULL arguments, a 65th lane of one rollout object. */
int ppo_carla_lane_create(ppo_carla_rollout_t* r, ppo_carla_lane_t** out);
int ppo_carla_lane_destroy(ppo_carla_lane_t* l);
/* :365-381 for one env. HOST pointers (pageable is fine): bev [C, IH, IW], meas [NM], vmeas [NV] (may
 * be NULL when NV = 0). Stores the observation row and next_done at [step, env], samples with
 * (env_base = env, step_id = iteration * T + step) — the keys of ppo_carla_rollout_act(step, env,
 * env + 1), whose stored results it reproduces bit for bit —, stores action / log-prob / value and
 * returns once action_host[0..A) holds the action. The bev row travels through the lane's pinned buffer
 * by one DMA straight into its storage row, the fp32 values as kernel arguments (k_carla_lane_in; by
 * copies when NM + NV exceeds its 62 floats), the action back by one copy followed by a wait on the
 * lane's stream only. Refused before any HIP call: NULL arguments, a (step, env) outside the storage. */
int ppo_carla_lane_act(ppo_carla_lane_t* l, int step, int env, const uint8_t* bev, const float* meas,
                       const float* vmeas, float next_done, float* action_host);
/* :385: rewards[step, env] = reward, asynchronous on the lane's stream */
int ppo_carla_lane_reward(ppo_carla_lane_t* l, int step, int env, float reward);
/* waits for everything the lane has queued */
int ppo_carla_lane_sync(ppo_carla_lane_t* l);

/* ---- test hook: a lane's k_carla_lane_in launch on caller rows ------------------------------------
 * meas_row[0..nm) = meas[0..nm), vmeas_row[0..nv) = vmeas[0..nv), *done_row = next_done,
 * *reward_row = reward: meas / vmeas are HOST arrays, the four rows device pointers; a NULL row is
 * skipped (vmeas_row with nv = 0, done_row, reward_row). nm + nv <= 62 travels as kernel arguments of
 * one launch; beyond that every value goes by a copy, as in a lane. Synchronises the stream. */
int ppo_carla_debug_lane_in(int nm, int nv, const float* meas, const float* vmeas, float next_done, float reward,
                            float* meas_row, float* vmeas_row, float* done_row, float* reward_row, void* stream);

/* ---- test hooks: the rollout object's gather launches on caller arrays (device pointers) ---------
 * k_carla_gather: dst[i, 0..row_bytes) = src[idx[i], 0..row_bytes) for i < n; rows are packed
 * (stride row_bytes), neither base pointer nor row_bytes need be a multiple of 16. n = 0 is a no-op.
 * k_carla_gather_f32: the same for nseg <= 8 fp32 arrays in one launch, rows of width[k] floats;
 * src / dst / width are HOST arrays of nseg entries (the pointers in them device pointers). */
int ppo_carla_debug_gather(long n, long row_bytes, const void* src, const int32_t* idx, void* dst, void* stream);
int ppo_carla_debug_gather_f32(long n, int nseg, const float* const* src, const int* width, const int32_t* idx,
                               float* const* dst, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PPO_CARLA_H */
