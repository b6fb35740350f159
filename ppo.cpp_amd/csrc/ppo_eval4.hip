// ppo_eval4.hip — k_eval4: the persistent policy evaluation kernel of the PPO agent (tanh-Normal,
// H = 64) on the device env, with the PPO wrapper chain fused in (ppo_evaluate_synth, mode = 2;
// ppo:589-626). k_eval (ppo_eval.hip) is the AC agent's; the event protocol is the same.
#include "ppo_rollout_common.hpp"

namespace {

// k_eval4's own blocks. load4_weights and trunk4 are shared with k_rollout4 (ppo_rollout_common.hpp:
// moving them left every kernel of ppo_rollout.hip byte-identical). The xv read, the head partials, the
// wrapper rows' prologue / epilogue and the env-and-wrapper phase below say what k_rollout4 has inline,
// and k_rollout4 does not call them: with any of them shared its device assembly changes (scalar spills
// of k_rollout4<24, 2, 4, 0> 165 -> 176), the shift that cost cfg2's rollout 3.8 % before, so
// its text stays as it is. The arithmetic they order is shared: env_lane_step, chee_*, wrap_*_at,
// ev_autoreset, ev_step_account.
//
// k_act4's xv of this lane (MFMA row j, columns 16 kb + 4 g .. + 3 of wave ks' k-blocks) from the
// workgroup's obs rows in LDS; rows past the block's R envs or past env E - 1 (rvalid false) are zero
template <int NTO, int NKW, int R>
PPO_DEV void xv4_from_rows(const float* XO, int O, int ks, int j, int g, bool rvalid, f4 (&xv)[NKW]) {
  constexpr int LDQ = NTO * 16 + 1;
#pragma unroll
  for (int q = 0; q < NKW; ++q) {
    const int kb = ks * NKW + q;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = 16 * kb + 4 * g + c;
      const float v = XO[min(j, R - 1) * LDQ + min(col, O - 1)];
      xv[q][c] = (kb < NTO && col < O && rvalid) ? v : 0.f;
    }
  }
}

// k_act4's actor head: wave ks' partial products of its 16 features of h2 into HP[ks] (the caller's
// barrier follows; the partials meet in the order ((HP[0] + HP[1]) + HP[2]) + HP[3])
template <int NHT>
PPO_DEV void head4_partials(const f4 (&hw)[NHT], f4 h2, float (*HP)[NHT * 16][kR4LDP], int ks, int j, int g) {
#pragma unroll
  for (int ht = 0; ht < NHT; ++ht) {
    f4 hp = f4{0.f, 0.f, 0.f, 0.f};
    hp = mfma16(hw[ht].x, h2.x, hp);
    hp = mfma16(hw[ht].y, h2.y, hp);
    hp = mfma16(hw[ht].z, h2.z, hp);
    hp = mfma16(hw[ht].w, h2.w, hp);
#pragma unroll
    for (int r = 0; r < 4; ++r) HP[ks][16 * ht + 4 * g + r][j] = hp[r];
  }
}

// The wrapper chain's state of a workgroup's R envs [row0, row0 + R) between global memory and LDS
// (the obs mean / var rows and the EV_W* slots), beside env_slots_load / env_slots_store and with
// their rules for rows past env E - 1
template <int R, int NT>
PPO_DEV void wrap_slots_load(float* EV, float* WOM, float* WOV, int ldq, const WrapArgs& w, int row0, int E, int O,
                             int tid) {
  for (int idx = tid; idx < R * O; idx += NT) {
    const int r = idx / O, f = idx - r * O, e = row0 + r;
    WOM[r * ldq + f] = e < E ? w.om[(long)e * O + f] : 0.0f;
    WOV[r * ldq + f] = e < E ? w.ov[(long)e * O + f] : 1.0f;
  }
  if (tid < R) {
    const int e = min(row0 + tid, E - 1);
    EV[EV_WOC * R + tid] = w.ocount[e];
    EV[EV_WRA * R + tid] = w.racc[e];
    EV[EV_WRM * R + tid] = w.rmean[e];
    EV[EV_WRV * R + tid] = w.rvar[e];
    EV[EV_WRC * R + tid] = w.rcount[e];
  }
}
template <int R, int NT>
PPO_DEV void wrap_slots_store(const float* EV, const float* WOM, const float* WOV, int ldq, const WrapArgs& w, int row0,
                              int E, int O, int tid) {
  for (int idx = tid; idx < R * O; idx += NT) {
    const int r = idx / O, f = idx - r * O, e = row0 + r;
    if (e < E) {
      w.om[(long)e * O + f] = WOM[r * ldq + f];
      w.ov[(long)e * O + f] = WOV[r * ldq + f];
    }
  }
  if (tid < R && row0 + tid < E) {
    const int e = row0 + tid;
    w.ocount[e] = EV[EV_WOC * R + tid];
    w.racc[e] = EV[EV_WRA * R + tid];
    w.rmean[e] = EV[EV_WRM * R + tid];
    w.rvar[e] = EV[EV_WRV * R + tid];
    w.rcount[e] = EV[EV_WRC * R + tid];
  }
}

// One env step of the workgroup's RR envs [row0, row0 + RR) that are below E, with the PPO wrapper
// chain fused (w.on), by all 256 threads between two barriers: 256 / RR lanes per env (one env within
// one wave), all RR envs at once. Actions come from ACT[r * 32 + 0..A-1]; the env state stays in Q,
// the agent's next input (the wrapped obs) in XO, the chain's running obs mean / var in WOM / WOV and
// its per-env scalars in the EV_W* slots. NormalizeReward and NormalizeObservation sit where the
// per-step env kernels apply them: the reward first (a reset step's reward 0 does not pass through
// NormalizeReward), then the observation. Lane 0 of each env calls lane0(e, r, outcome, wrapped
// reward) once per step, the caller's own part: the evaluation's episode event.
template <int KIND, int NTO, int RR, typename F>
PPO_DEV void env4_step(float* EV, float* XO, float* Q, float* WOM, float* WOV, const float* ACT, const WrapArgs& w,
                       float lo, float hi, int row0, int E, int O, int A, int tid, F&& lane0) {
  constexpr int R = RR, OP = NTO * 16, LPE = kR4Threads / RR, LDQ = OP + 1;
  constexpr int NCE = (OP + LPE - 1) / LPE, kEnvGroup = 12;
  int* EVI = reinterpret_cast<int*>(EV);
  (void)EVI;
  if constexpr (KIND != PSYN_CHEETAH) {
    // a kind with a DevEnv (k_env_step arithmetic): lane 0 of each env's lane group steps the env
    // from its actions ACT[r * 32 + 0..A-1] (written by other lanes before the caller's barrier). The
    // step's termination flag goes to NormalizeReward (a reset step's reward 0 does not pass through
    // it); the raw observation lies in XO, which the wrapper chain normalises where it lies.
#pragma clang fp contract(off)
    const int r = tid / LPE, i0 = tid % LPE, e = row0 + r;
    if (i0 == 0 && e < E) {
      float* xo = XO + r * LDQ;
      const EnvLaneOut o = env_lane_step<KIND, R>(EV, r, Q + r * LDQ, xo, ACT + r * 32, lo, hi);
      lane0(e, r, o,
            (w.on && !o.reset) ? wrap_reward_at(EV + EV_WRA * R + r, EV + EV_WRM * R + r, EV + EV_WRV * R + r,
                                                EV + EV_WRC * R + r, w.gamma, o.reward, o.term)
                               : o.reward);
      if (w.on) {
        float* om = WOM + r * LDQ;
        float* ov = WOV + r * LDQ;
        const float oc = EV[EV_WOC * R + r];
        for (int i = 0; i < DevEnv<KIND>::O; ++i) xo[i] = wrap_obs_at(om + i, ov + i, oc, xo[i]);
        EV[EV_WOC * R + r] = oc + 1.0f;
      }
    }
  } else {
    // the synthetic cheetah (k_synth_step / _wide arithmetic) over the env's LPE lanes; lane 0 does
    // the reward and the episode contract (chee_lanes_step's, with the wrapper chain in between)
#pragma clang fp contract(off)
    const int r = tid / LPE, i0 = tid % LPE, e = row0 + r;
    if (e < E) {
      const bool reset = EVI[EV_AR * R + r] != 0;
      float* q = Q + r * LDQ;
      float* xo = XO + r * LDQ;
      float* om = WOM + r * LDQ;
      float* ov = WOV + r * LDQ;
      const float* ar = ACT + r * 32;
      const float oc = EV[EV_WOC * R + r];  // read by every lane before lane 0 stores oc + 1
      if (reset) {
        const uint32_t rs = (uint32_t)EVI[EV_RSEED * R + r], rc = (uint32_t)EVI[EV_RCOUNT * R + r];
#pragma unroll
        for (int c = 0; c < NCE; ++c) {
          const int i = LPE * c + i0;
          if (i < O) {
            const float v = chee_reset_elem(rc, rs, i);
            q[i] = v;
            xo[i] = w.on ? wrap_obs_at(om + i, ov + i, oc, v) : v;
          }
        }
        if (i0 == 0) {
          if (w.on) EV[EV_WOC * R + r] = oc + 1.0f;
          ev_autoreset<R>(EV, r, rc);
          lane0(e, r, EnvLaneOut{0.0f, 0.0f, false, true, 0.0f, 0}, 0.0f);
        }
      } else {
        // Groups of up to 12 elements per lane: every LDS operand of a group is read before any
        // of its results is written (independent element chains; interleaved loads and stores
        // through possibly aliasing LDS pointers would serialise them). One env's LPE lanes are in
        // one wave, so a q[i + 1] read precedes the neighbour's store in program order; the wrap
        // to q[0] reads the value from before the step.
        const float q0_old = q[0];
        const Recip rtot = recip_of(oc + 1.0f);
        float q0_new = 0.0f;
        int ai = i0 % A;
        const int astep = LPE % A;
#pragma unroll
        for (int c0 = 0; c0 < NCE; c0 += kEnvGroup) {
          float qo[kEnvGroup], qn[kEnvGroup], wm[kEnvGroup], wv[kEnvGroup], ac[kEnvGroup];
#pragma unroll
          for (int u = 0; u < kEnvGroup; ++u) {
            if (c0 + u < NCE) {
              const int i = min(LPE * (c0 + u) + i0, O - 1);
              qo[u] = q[i];
              qn[u] = i + 1 < O ? q[i + 1] : q0_old;
              ac[u] = ar[ai];
              ai += astep;
              ai = ai >= A ? ai - A : ai;
              if (w.on) {
                wm[u] = om[i];
                wv[u] = ov[i];
              }
            }
          }
          float nq[kEnvGroup], xn[kEnvGroup];
#pragma unroll
          for (int u = 0; u < kEnvGroup; ++u) {
            if (c0 + u < NCE) {
              nq[u] = chee_next_q(qo[u], chee_clip(ac[u], lo, hi), qn[u]);
              xn[u] = w.on ? wrap_obs_at_r(&wm[u], &wv[u], oc, rtot, nq[u]) : nq[u];
            }
          }
          if (c0 == 0) q0_new = nq[0];
#pragma unroll
          for (int u = 0; u < kEnvGroup; ++u) {
            const int i = LPE * (c0 + u) + i0;
            if (c0 + u < NCE && i < O) {
              q[i] = nq[u];
              xo[i] = xn[u];
              if (w.on) {
                om[i] = wm[u];
                ov[i] = wv[u];
              }
            }
          }
        }
        if (i0 == 0) {
          if (w.on) EV[EV_WOC * R + r] = oc + 1.0f;
          EnvLaneOut out{chee_reward_clip(q0_new, q0_old, ar, A, lo, hi), 0.0f, false, false, 0.0f, 0};
          ev_step_account<R>(EV, r, CHEE_MAX_STEPS, out);
          lane0(e, r, out,
                w.on ? wrap_reward_at(EV + EV_WRA * R + r, EV + EV_WRM * R + r, EV + EV_WRV * R + r,
                                      EV + EV_WRC * R + r, w.gamma, out.reward, 0.0f)
                     : out.reward);
        }
      }
    }
  }
}

}  // namespace

// One persistent launch per chunk of env steps for the PPO agent (two 64-wide tanh trunks, Normal
// head) on any device env kind, with the PPO wrapper chain (env.w.on) or without. k_rollout4's
// geometry: 256 threads, RR = 4 or 16 envs per workgroup, wave ks keeps its K-slice of W1 (all 64 outputs), its tile of W2 and its head
// tile in registers for the whole chunk; layer 1's four K-slice partials meet in LDS in the order
// ((P0 + P1) + P2) + P3 (trunk4: k_act4's arithmetic). Per step: the wrapped obs of the block's envs
// (XO) -> xv -> trunk -> head partials -> mean | mean + z sd -> ACT -> env4_step (clip, env step,
// NormalizeReward, NormalizeObservation on the LDS rows) -> XO. Against k_rollout4 it has no rollout
// stores, no log-prob (so no var / log sd registers), and under PPO_MEAN no Philox / Box-Muller draws;
// the reward still passes through NormalizeReward, whose state the per-step path updates too. The
// only global writes of the loop are the episode events. The env state, the wrapper chain's state
// and the obs of the envs [0, nE) come in with the prologue and go back with the epilogue: the next
// chunk, a later psyn_step or a rollout continues from them. On a context whose act kernel is k_act4
// every action, observation, return and state word is bitwise the per-step path's.
// LDS (floats): P1 4 x 64 x 17, H1 16 x 68, HP 4 x NHP x 17, XO | Q | WOM | WOV RR x (OP + 1) each,
// ACT RR x 32, EV 15 x RR: 27 952 bytes at <1, 1, 4>, 55 856 at <24, 2, 4>, 132 032 at <24, 2, 16>.
template <int NTO, int NHT, int RR, int KIND = PSYN_CHEETAH>
__global__ __launch_bounds__(256) void k_eval4(EvalArgs a) {
  static_assert(psyn_kind_tiles_ok<KIND, NTO, NHT>(), PSYN_KIND_TILES_MSG);
  static_assert(RR == 4 || RR == 16, "k_eval4: 4 or 16 envs per workgroup");
  constexpr int H = kR4H, R = RR, OP = NTO * 16, NKW = (NTO + 3) / 4, NHP = NHT * 16;
  constexpr int LDQ = Roll4Geo<NTO, NHT>::LDQ;
  __shared__ float P1[4][H][kR4LDP];
  __shared__ __attribute__((aligned(16))) float H1[kR4Rows][kR4LDH];
  __shared__ float HP[4][NHP][kR4LDP];
  __shared__ float XO[R * LDQ];   // the agent's input of the current step (the wrapped obs)
  __shared__ float Q[R * LDQ];    // env state q
  __shared__ float ACT[R * 32];
  __shared__ float EV[EV_NSLOT * R];
  __shared__ float WOM[R * LDQ];  // the wrapper chain's running obs mean / var of the block's envs
  __shared__ float WOV[R * LDQ];
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 15, g = lane >> 4, ks = tid >> 6;
  const PackedLayout& K = a.K;
  const TrunkDev& T = K.tr[1];
  const float* __restrict__ P = a.P;
  const PBuf pb = make_pbuf(P, K.size);
  const int row0 = blockIdx.x * R, O = K.O, A = K.A, E = a.nE;  // the evaluated envs [0, nE)
  const WrapArgs& w = a.env.w;

  // ---- prologue: resident weights, per-item head parameters, env and wrapper state of this block ----
  f4 wa[NKW][4], w2v[4], hw[NHT];
  load4_weights<NTO, NKW>(make_pbuf(a.WSW, (int)sw_size(H, OP)), lane, ks, wa, w2v);
  const f4 b1 = pld4(pb, T.b1 + 16 * ks + 4 * g, 0);
  const f4 b2 = pld4(pb, T.b2 + 16 * ks + 4 * g, 0);
#pragma unroll
  for (int ht = 0; ht < NHT; ++ht) {
    const int h = 16 * ht + j;
    const f4 wv = pld4(pb, K.aW3 + min(h, A - 1) * H + 16 * ks + 4 * g, 0);
    hw[ht] = h < A ? wv : f4{0.f, 0.f, 0.f, 0.f};
  }
  // item tid + 256 u is (env idx / A of the block, action idx % A): its head bias and std (k_act4's
  // expf of the log std) are constant over the chunk
  constexpr int NI = (R * NHP + kR4Threads - 1) / kR4Threads;
  float i_b3[NI], i_sd[NI];
#pragma unroll
  for (int u = 0; u < NI; ++u) {
    const int ia = min(tid + kR4Threads * u, R * A - 1) % A;
    i_b3[u] = P[K.ab3 + ia];
    i_sd[u] = expf(P[K.logstd + ia]);
  }
  env_slots_load<R, kR4Threads>(EV, XO, Q, LDQ, a.env, a.obs, nullptr, row0, E, O, tid);
  if (w.on) wrap_slots_load<R, kR4Threads>(EV, WOM, WOV, LDQ, w, row0, E, O, tid);
  __syncthreads();
  const SampleKey key = sample_key(a.seed, a.rank);
  const bool sample = a.mode == PPO_SAMPLE;
  const bool rvalid = j < R && row0 + j < E;  // MFMA tile row j is one of this block's evaluated envs

  for (int t = 0; t < a.T; ++t) {
    const long step_id = a.step0 + t;
    f4 xv[NKW];
    xv4_from_rows<NTO, NKW, R>(XO, O, ks, j, g, rvalid, xv);
    // PPO_SAMPLE: the step's Normal draws do not depend on the network; issued under the layer-1 MFMAs
    float nz[NI];
#pragma unroll
    for (int u = 0; u < NI; ++u) nz[u] = 0.f;
    const f4 h2 = trunk4<NTO, NKW>(xv, wa, w2v, b1, b2, P1, H1, ks, j, g, [&] {
      if (sample) {
#pragma unroll
        for (int u = 0; u < NI; ++u) {
          const int idx = min(tid + kR4Threads * u, R * A - 1), ir = idx / A, ia = idx - ir * A;
          nz[u] = normal_z(key, (long)(row0 + ir), step_id, ia);
        }
      }
    });
    head4_partials<NHT>(hw, h2, HP, ks, j, g);
    __syncthreads();
    // ---- the action (k_act4's outputs stage): the head's mean, or mean + z sd ----
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      const int idx = tid + kR4Threads * u;
      if (idx < R * A) {
        const int ir = idx / A, ia = idx - ir * A;
        const float mu = (((HP[0][ia][ir] + HP[1][ia][ir]) + HP[2][ia][ir]) + HP[3][ia][ir]) + i_b3[u];
        const float sd = i_sd[u];
        float act;
        if (sample) act = mu + nz[u] * sd;
        else act = mu;
        ACT[ir * 32 + ia] = act;
      }
    }
    __syncthreads();
    // ---- env step with the wrapper chain; an episode that terminates or is truncated, on whatever
    // step, is one event ----
    env4_step<KIND, NTO, RR>(EV, XO, Q, WOM, WOV, ACT, w, a.lo, a.hi, row0, E, O, A, tid,
                             [&](int e, int, const EnvLaneOut& o, float) {
                               if (o.fin) {
                                 const unsigned slot = atomicAdd(a.count, 1u);
                                 if (slot < (unsigned)a.cap) a.ev[slot] = EvalEvent{a.k0 + t, e, o.epl, o.epr};
                               }
                             });
    __syncthreads();
  }
  // ---- epilogue: the obs, the env state and the wrapper state back to HBM ----
  env_slots_store<R, kR4Threads>(EV, XO, Q, LDQ, a.env, a.obs, nullptr, row0, E, O, tid);
  if (w.on) wrap_slots_store<R, kR4Threads>(EV, WOM, WOV, LDQ, w, row0, E, O, tid);
}

// 0 when k_eval4 covers the agent (PPO agent, H = 64, A <= 32, OP / 16 in {1, 2, 7, 24}): for this
// agent exactly rollout_supported's set
int eval4_supported(const PackedLayout& K) {
  const int nto = K.OP / 16;
  return (K.kind == PPO_NET_TANH_NORMAL && K.H == 64 && K.A <= 32 && (nto == 1 || nto == 2 || nto == 7 || nto == 24)) ? 0 : -1;
}

// 4 envs per workgroup while that still fits one workgroup per CU, 16 beyond (launch_rollout4_t's
// rule, on the evaluated envs)
template <int NTO, int NHT, int KIND = PSYN_CHEETAH>
static int launch_eval4_t(const EvalArgs& a, hipStream_t s) {
  // the CU count of the current device, asked once per device and thread: chunk_steps = 1 launches
  // once per env step
  thread_local int ncu_dev = -1, ncu = 256;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != ncu_dev) {
    ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    ncu_dev = dev;
  }
  if ((a.nE + 3) / 4 <= ncu)
    hipLaunchKernelGGL((k_eval4<NTO, NHT, 4, KIND>), dim3((a.nE + 3) / 4), dim3(kR4Threads), 0, s, a);
  else
    hipLaunchKernelGGL((k_eval4<NTO, NHT, 16, KIND>), dim3((a.nE + 15) / 16), dim3(kR4Threads), 0, s, a);
  return 0;
}

int launch_eval4(const EvalArgs& a, hipStream_t s) {
  if (eval4_supported(a.K) != 0 || a.nE <= 0 || a.T <= 0) return -1;
  if (a.mode != PPO_SAMPLE && a.mode != PPO_MEAN) return -1;
  if (a.env.kind != PSYN_CHEETAH)  // a kind with a DevEnv, at its own tile shape and action width; no kind: -1
    return dispatch_env_kind(a.env.kind, [&](auto KIND_) {
      constexpr int KIND = decltype(KIND_)::value;
      using D = DevEnv<KIND>;
      return (a.K.OP == 16 * D::NTO && a.K.A == D::A) ? launch_eval4_t<D::NTO, D::NHT, KIND>(a, s) : -1;
    });
  const int nht = (a.K.A + 15) / 16;
  switch (a.K.OP / 16) {
    case 1: return nht == 1 ? launch_eval4_t<1, 1>(a, s) : launch_eval4_t<1, 2>(a, s);
    case 2: return nht == 1 ? launch_eval4_t<2, 1>(a, s) : launch_eval4_t<2, 2>(a, s);
    case 7: return nht == 1 ? launch_eval4_t<7, 1>(a, s) : launch_eval4_t<7, 2>(a, s);
    case 24: return nht == 1 ? launch_eval4_t<24, 1>(a, s) : launch_eval4_t<24, 2>(a, s);
  }
  return -1;
}
