// ppo_eval.hip — policy evaluation on the device env (ppo_evaluate_synth; ac:965-1001, ppo:589-626).
//
//  * k_eval: one persistent launch per chunk of env steps for the AC agent (LayerNorm-Beta, H = 256,
//    OP <= 32, env without wrappers). One workgroup owns 16 envs for all T steps of the chunk, the
//    actor's W1 / W2 slices resident in registers (k_rollout's geometry and blocks,
//    ppo_rollout_common.hpp): obs -> actor -> mean | roach | sample -> clip -> env step -> obs inside
//    the kernel with LDS barriers only. No critic, no log-probs, no rollout stores: the only global
//    writes in the loop are the episode events. The actor's chain is k_act3's and the env step
//    k_synth_step's, op for op, so every action, observation and return is bitwise the per-step
//    path's (ppo_get_action_and_value + psyn_step; tests/test_gpu_eval.py).
//  * k_eval_record: the per-step path's event recorder, one launch after each psyn_step.
// Events go to a global buffer through a vector atomic counter, in any order; the host sorts them by
// (step, env) (ppo_eval_events.hpp).
#include "ppo_rollout_common.hpp"

// KIND: the device env's kind, compile-time as in k_rollout
template <int NTO, int NHT, int KIND = PSYN_CHEETAH>
__global__ __launch_bounds__(512) void k_eval(EvalArgs a) {
  static_assert(psyn_kind_tiles_ok<KIND, NTO, NHT>(), PSYN_KIND_TILES_MSG);
  using GE = RollGeo<NTO, NHT>;
  constexpr int OP = GE::OP, LDX = GE::LDX, LDP = GE::LDP, LDQ = GE::LDQ, R = kRows;
  constexpr int NCH = (OP + 31) / 32;  // 32-dim chunks of the env state per env lane group
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* XS = lds + GE::oXS;
  float* PRE = lds + GE::oPRE;
  float* ITM = lds + GE::oITM;
  float* XO = lds + GE::oXO;
  float* Q = lds + GE::oQ;
  float* NRM = lds + GE::oNRM;
  float* ACT = lds + GE::oACT;
  float* EV = lds + GE::oENV;
  int* EVI = reinterpret_cast<int*>(EV);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PackedLayout& K = a.K;
  const float* __restrict__ P = a.P;
  const PBuf pb = make_pbuf(P, K.size);
  const int O = K.O, A = K.A, E = a.nE;  // the evaluated envs [0, nE); the env's other envs are not touched
  const int row0 = blockIdx.x * R;
  const SynthArgs& sv = a.env;

  // ---- prologue: resident weights, staged parameters, env state of this block ----
  f4 w1[NTO][2], w2[16][2];
  load_weight_slices<NTO>(make_pbuf(a.WSW, (int)sw_size(256, OP)), wave, lane, w1, w2);
  stage_params<GE::NHP>(K, K.tr[1], pb, 1, lds + GE::oSP, lds + GE::oHBIAS, tid);
  for (int f = tid; f < OP; f += kActThreads) {
    NRM[f] = f < O ? P[K.omean + f] : 0.0f;
    NRM[OP + f] = f < O ? P[K.ostd + f] : 1.0f;
  }
  for (int idx = tid; idx < R * O; idx += kActThreads) {
    const int r = idx / O, f = idx - r * O, e = row0 + r;
    XO[r * LDQ + f] = e < E ? a.obs[(long)e * O + f] : 0.0f;
    Q[r * LDQ + f] = e < E ? sv.q[(long)e * O + f] : 0.0f;
  }
  if (tid < R) {
    const int e = min(row0 + tid, E - 1);
    EVI[EV_AR * R + tid] = sv.autoreset[e];
    EVI[EV_T * R + tid] = sv.t[e];
    EVI[EV_RSEED * R + tid] = (int)sv.rseed[e];
    EVI[EV_RCOUNT * R + tid] = (int)sv.rcount[e];
    EV[EV_EPR * R + tid] = sv.ep_ret[e];
    EVI[EV_EPL * R + tid] = sv.ep_len[e];
    EV[EV_FR * R + tid] = sv.fin_ret[e];
    EV[EV_FL * R + tid] = sv.fin_len[e];
    EV[EV_FC * R + tid] = sv.fin_cnt[e];
  }
  lds_barrier();
  const SampleKey key = sample_key(a.seed, a.rank);
  const float hi = P[K.hi], lo = P[K.lo];
  const bool sample = a.mode == PPO_SAMPLE;
  // this thread's Beta item (row, action, alpha | beta), spread over the waves as in k_rollout
  const int bper = (R * A * 2 + kActWaves - 1) / kActWaves;
  const int bitem = lane < bper ? wave * bper + lane : R * A * 2;

  for (int t = 0; t < a.T; ++t) {
    const long step_id = a.step0 + t;
    // ---- normalised rows into XS (k_act3 order) ----
    for (int idx = tid; idx < R * OP; idx += kActThreads) {
      const int r = idx / OP, f = idx - r * OP, e = row0 + r;
      const bool valid = e < E && f < O;
      const float x = valid ? XO[r * LDQ + f] : 0.0f;
      XS[r * LDX + f] = valid ? (x - NRM[f]) / NRM[OP + f] : x;
    }
    lds_barrier();
    // PPO_SAMPLE: the first Marsaglia-Tsang attempt's draws do not depend on the network; computed
    // under layer 2's MFMAs (gamma_mt_d0 with them is gamma_mt, bitwise)
    GammaDraw gd0 = GammaDraw{0.f, 0.f};
    const auto draw0 = [&] {
      if (sample && bitem < R * A * 2) {
        const int which = bitem & 1, ra = bitem >> 1, r = ra / A, ai = ra - r * A;
        gd0 = gamma_draw(key, (long)(row0 + r), step_id, 0x10000u + (uint32_t)(ai * 2 + which) * 64u);
      }
    };
    trunk_rows<NTO, NHT>(w1, w2, lds, 2 * A, tid, draw0);
    // ---- concentrations (k_act3 stage 1) and the action on [0, 1] (stage 2) ----
    if (bitem < R * A * 2) {
      const int which = bitem & 1, ra = bitem >> 1, r = ra / A, ai = ra - r * A;
      const float c = softplusf_(PRE[r * LDP + ai + which * A]) + 1.0f;
      float gs = 0.f;
      if (sample) gs = gamma_mt_d0(c, gd0, key, (long)(row0 + r), step_id, 0x10000u + (uint32_t)(ai * 2 + which) * 64u);
      float* it = ITM + ((r * A + ai) * 2 + which) * 4;
      it[0] = c;
      it[1] = gs;
    }
    lds_barrier();
    for (int idx = tid; idx < R * A; idx += kActThreads) {
      const int r = idx / A, ai = idx - r * A;
      const float* ia = ITM + (idx * 2 + 0) * 4;
      const float* ib = ITM + (idx * 2 + 1) * 4;
      const float al = ia[0], be = ib[0];
      float s01;
      if (a.mode == PPO_MEAN) s01 = al / (al + be);
      else if (a.mode == PPO_ROACH) s01 = beta_roach01(al, be);
      else s01 = beta_sample01(ia[1], ib[1]);
      ACT[r * 24 + ai] = (s01 - 0.0f) / (1.0f - 0.0f) * (hi - lo) + lo;
    }
    lds_barrier();
    // ---- env step: 32 lanes per env; a finished episode is one event ----
    if constexpr (KIND != PSYN_CHEETAH) {
      // a kind with a DevEnv (k_env_step arithmetic): lane 0 of each env's lane group steps the env
      // from its actions ACT[r * 24 + 0..A-1]; an episode that terminates or is truncated, on whatever
      // step, is one event
#pragma clang fp contract(off)
      const int r = tid >> 5, i0 = tid & 31, e = row0 + r;
      if (i0 == 0 && e < E) {
        const EnvLaneOut o = env_lane_step<KIND, R>(EV, r, Q + r * LDQ, XO + r * LDQ, ACT + r * 24, a.lo, a.hi);
        if (o.fin) {
          const unsigned slot = atomicAdd(a.count, 1u);
          if (slot < (unsigned)a.cap) a.ev[slot] = EvalEvent{a.k0 + t, e, o.epl, o.epr};
        }
      }
    } else {
      // the synthetic cheetah (k_synth_step arithmetic)
#pragma clang fp contract(off)
      const int r = tid >> 5, i0 = tid & 31, e = row0 + r;
      const bool live = e < E;
      const bool reset = EVI[EV_AR * R + r] != 0;
      float* q = Q + r * LDQ;
      float* xo = XO + r * LDQ;
      const float* ar = ACT + r * 24;
      if (live && reset) {
        const uint32_t rs = (uint32_t)EVI[EV_RSEED * R + r], rc = (uint32_t)EVI[EV_RCOUNT * R + r];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int i = 32 * c + i0;
          if (i < O) {
            uint32_t rr[4];
            philox4x32(rc, (uint32_t)i, 0u, 0u, rs, 0x5EED5EEDu, rr);
            const float v = (0.1f * ((2.0f * u01(rr[0])) - 1.0f));
            q[i] = v;
            xo[i] = v;
          }
        }
        if (i0 == 0) {
          EVI[EV_RCOUNT * R + r] = (int)(rc + 1);
          EVI[EV_T * R + r] = 0;
          EV[EV_EPR * R + r] = 0.0f;
          EVI[EV_EPL * R + r] = 0;
          EVI[EV_AR * R + r] = 0;
        }
      } else if (live) {
        float qo[NCH], qn[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int i = 32 * c + i0;
          qo[c] = i < O ? q[i] : 0.0f;
          qn[c] = i < O ? q[i + 1 < O ? i + 1 : 0] : 0.0f;
        }
        float q0_new = 0.0f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int i = 32 * c + i0;
          if (i < O) {
            const float ai = fminf(fmaxf(ar[i % A], a.lo), a.hi);
            const float nq = __fmaf_rn(0.9f, qo[c], __fmaf_rn(0.1f, ai, (0.05f * qn[c])));
            q[i] = nq;
            xo[i] = nq;
            if (c == 0) q0_new = nq;
          }
        }
        if (i0 == 0) {
          const float vel = ((q0_new - qo[0]) / 0.05f);
          float ctrl = 0.0f;
          for (int k = 0; k < A; ++k) {
            const float ak = fminf(fmaxf(ar[k], a.lo), a.hi);
            ctrl = (ctrl + ((0.1f * ak) * ak));
          }
          const float rw = (vel - ctrl);
          const int tt = EVI[EV_T * R + r] + 1;
          EVI[EV_T * R + r] = tt;
          const bool tr = tt >= 1000;
          const float epr = (EV[EV_EPR * R + r] + rw);
          EV[EV_EPR * R + r] = epr;
          const int epl = EVI[EV_EPL * R + r] + 1;
          EVI[EV_EPL * R + r] = epl;
          if (tr) {
            EV[EV_FR * R + r] += epr;
            EV[EV_FL * R + r] += (float)epl;
            EV[EV_FC * R + r] += 1.0f;
            const unsigned slot = atomicAdd(a.count, 1u);
            if (slot < (unsigned)a.cap) a.ev[slot] = EvalEvent{a.k0 + t, e, epl, epr};
          }
          EVI[EV_AR * R + r] = tr ? 1 : 0;
        }
      }
    }
    lds_barrier();
  }
  // ---- epilogue: the obs and the env state back to HBM (the next chunk continues from them) ----
  for (int idx = tid; idx < R * O; idx += kActThreads) {
    const int r = idx / O, f = idx - r * O, e = row0 + r;
    if (e < E) {
      a.obs[(long)e * O + f] = XO[r * LDQ + f];
      sv.q[(long)e * O + f] = Q[r * LDQ + f];
    }
  }
  if (tid < R && row0 + tid < E) {
    const int e = row0 + tid;
    sv.autoreset[e] = EVI[EV_AR * R + tid];
    sv.t[e] = EVI[EV_T * R + tid];
    sv.rseed[e] = (uint32_t)EVI[EV_RSEED * R + tid];
    sv.rcount[e] = (uint32_t)EVI[EV_RCOUNT * R + tid];
    sv.ep_ret[e] = EV[EV_EPR * R + tid];
    sv.ep_len[e] = EVI[EV_EPL * R + tid];
    sv.fin_ret[e] = EV[EV_FR * R + tid];
    sv.fin_len[e] = EV[EV_FL * R + tid];
    sv.fin_cnt[e] = EV[EV_FC * R + tid];
  }
}

// the per-step path's recorder, after psyn_step of evaluation step `step`: an env whose step ended
// its episode (done = 1) produces one event from its RecordEpisodeStatistics state
__global__ __launch_bounds__(256) void k_eval_record(SynthArgs env, const float* __restrict__ done, int nE,
                                                     long long step, EvalEvent* ev, unsigned* count, int cap) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nE || done[e] == 0.0f) return;
  const unsigned slot = atomicAdd(count, 1u);
  if (slot < (unsigned)cap) ev[slot] = EvalEvent{step, e, env.ep_len[e], env.ep_ret[e]};
}

void launch_eval_record(const SynthArgs& env, const float* done, int nE, long long step, EvalEvent* ev,
                        unsigned* count, int cap, hipStream_t s) {
  hipLaunchKernelGGL(k_eval_record, dim3((nE + 255) / 256), dim3(256), 0, s, env, done, nE, step, ev, count, cap);
}

// 0 when the persistent evaluation kernel covers the agent (AC agent, H = 256, one head tile, OP <= 32)
int eval_supported(const PackedLayout& K) {
  return (K.kind == PPO_NET_LN_BETA && K.H == 256 && 2 * K.A <= 16 && (K.OP == 16 || K.OP == 32)) ? 0 : -1;
}

template <int NTO, int KIND = PSYN_CHEETAH>
static int launch_eval_t(const EvalArgs& a, hipStream_t s) {
  using GE = RollGeo<NTO, 1>;
  const size_t lds = (size_t)GE::total * sizeof(float);
  static const bool ok = hipFuncSetAttribute((const void*)k_eval<NTO, 1, KIND>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds) == hipSuccess;
  if (!ok) return -2;
  hipLaunchKernelGGL((k_eval<NTO, 1, KIND>), dim3((a.nE + kRows - 1) / kRows), dim3(kActThreads), lds, s, a);
  return 0;
}

int launch_eval(const EvalArgs& a, hipStream_t s) {
  if (eval_supported(a.K) != 0 || a.env.w.on || a.nE <= 0 || a.T <= 0) return -1;
  if (a.mode != PPO_SAMPLE && a.mode != PPO_MEAN && a.mode != PPO_ROACH) return -1;
  if (a.env.kind != PSYN_CHEETAH)  // a kind with a DevEnv, at its own tile shape and action width; no kind: -1
    return dispatch_env_kind(a.env.kind, [&](auto KIND_) {
      constexpr int KIND = decltype(KIND_)::value;
      using D = DevEnv<KIND>;
      static_assert(D::NHT == 1, "k_eval: one head tile");
      return (a.K.OP == 16 * D::NTO && a.K.A == D::A) ? launch_eval_t<D::NTO, KIND>(a, s) : -1;
    });
  return a.K.OP == 16 ? launch_eval_t<1>(a, s) : launch_eval_t<2>(a, s);
}
