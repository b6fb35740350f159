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
  env_slots_load<R, kActThreads>(EV, XO, Q, LDQ, sv, a.obs, nullptr, row0, E, O, tid);
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
        const BetaItem bi = beta_item(bitem, A);
        gd0 = gamma_draw(key, (long)(row0 + bi.r), step_id, bi.db);
      }
    };
    trunk_rows<NTO, NHT>(w1, w2, lds, 2 * A, tid, draw0);
    // ---- concentrations (k_act3 stage 1) and the action on [0, 1] (stage 2) ----
    if (bitem < R * A * 2) {
      const BetaItem bi = beta_item(bitem, A);
      const float c = softplusf_(PRE[bi.r * LDP + bi.ai + bi.which * A]) + 1.0f;
      float gs = 0.f;
      if (sample) gs = gamma_mt_d0(c, gd0, key, (long)(row0 + bi.r), step_id, bi.db);
      float* it = ITM + ((bi.r * A + bi.ai) * 2 + bi.which) * 4;
      it[0] = c;
      it[1] = gs;
    }
    lds_barrier();
    for (int idx = tid; idx < R * A; idx += kActThreads) {
      const int r = idx / A, ai = idx - r * A;
      const float* ia = ITM + (idx * 2 + 0) * 4;
      const float* ib = ITM + (idx * 2 + 1) * 4;
      const float al = ia[0], be = ib[0];
      // own three-way switch (no PPO_GIVEN here; with beta_unit k_eval measured over its speed bound)
      float s01;
      if (a.mode == PPO_MEAN) s01 = al / (al + be);
      else if (a.mode == PPO_ROACH) s01 = beta_roach01(al, be);
      else s01 = beta_sample01(ia[1], ib[1]);
      ACT[r * 24 + ai] = beta_action(s01, lo, hi);
    }
    lds_barrier();
    // ---- env step: 32 lanes per env (k_rollout's); an episode that terminates or is truncated, on
    // whatever step, is one event ----
    {
      const int r = tid >> 5, i0 = tid & 31, e = row0 + r;
      if (e < E) {
        env_lanes_step<KIND, R, NCH>(EV, r, i0, O, A, Q + r * LDQ, XO + r * LDQ, ACT + r * 24, a.lo, a.hi,
                                     [&](const EnvLaneOut& o) {
                                       if (o.fin) {
                                         const unsigned slot = atomicAdd(a.count, 1u);
                                         if (slot < (unsigned)a.cap) a.ev[slot] = EvalEvent{a.k0 + t, e, o.epl, o.epr};
                                       }
                                     });
      }
    }
    lds_barrier();
  }
  // ---- epilogue: the obs and the env state back to HBM (the next chunk continues from them) ----
  env_slots_store<R, kActThreads>(EV, XO, Q, LDQ, sv, a.obs, nullptr, row0, E, O, tid);
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
