// ppo_carla_rollout.hip — the CaRL trainer's rollout storage, GAE and minibatch epoch loop
// (ac_ppo_carla.cpp:284-621) beside a ppo_carla_t: include/ppo_carla.h, "rollout storage, GAE and the
// epoch loop". The agent computes (ppo_carla_forward / ppo_carla_update, ppo_carla.hip); this unit owns
// the [T, E, ...] storage, the permutations and the row gather that feeds each minibatch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstring>
#include <string>

#include "../../include/ppo_carla.h"
#include "../../include/ppo_hip.h"
#include "ppo_carla_internal.hpp"
#include "ppo_kernels.hpp"

namespace {

// ------------------------------------------------------------------------------------------
// k_carla_gather: dst[i, :] = src[idx[i], :], rows of row_bytes bytes
// ------------------------------------------------------------------------------------------
// A pure stream: every byte is read once and written once, nothing is reused. A row is cut into
// chunks of kGatherChunk bytes, one workgroup per (row, chunk): with V = uint4 every lane moves one
// 16-byte vector (1 KiB per wave-instruction, the widest global access) and the chip's occupancy, not a
// loop, keeps loads in flight. Measured at 2 048 rows of 552 960 bytes: 4 KiB chunks, one
// per workgroup, beat 16 KiB chunks with four loads per lane ahead of the stores and any grid-stride cap
// (0.41 against 0.43-0.44 ms), and eight loads per lane were slower (0.50-0.57 ms). Consecutive
// workgroups take consecutive chunks of one row.
//
// Width V per row: source and destination row must sit at the same offset modulo sizeof(V) for
// V-wide accesses to be aligned on both sides. Rows whose two addresses agree modulo 16 copy in
// uint4 (every row when both bases are 16-byte aligned and row_bytes is a multiple of 16: the bev
// storage), modulo 4 in uint32, the rest bytewise. The head — the bytes before the destination's
// first V boundary — and the tail after the last whole V are copied bytewise by the row's chunk 0.
// The choice is uniform over a workgroup (it depends on the row only): no divergence.
constexpr long kGatherChunk = 4096;
constexpr int kGatherThreads = 256;
// beyond that many (row, chunk) items the grid strides (a launch holds fewer than 2^32 threads)
constexpr long kGatherMaxBlocks = 1L << 22;

template <typename V>
__device__ __forceinline__ void gather_chunk(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, long bytes,
                                             long chunk) {
  constexpr long W = (long)sizeof(V), EPC = kGatherChunk / W;
  const long tid = threadIdx.x;
  long h = (long)((0 - (uintptr_t)d) & (uintptr_t)(W - 1));
  if (h > bytes) h = bytes;
  const long nv = (bytes - h) / W, t = bytes - h - nv * W;
  const V* __restrict__ sv = reinterpret_cast<const V*>(s + h);
  V* __restrict__ dv = reinterpret_cast<V*>(d + h);
  const long end = nv < (chunk + 1) * EPC ? nv : (chunk + 1) * EPC;
  for (long v = chunk * EPC + tid; v < end; v += kGatherThreads) dv[v] = sv[v];  // one trip for V = uint4
  if (chunk == 0 && W > 1) {  // h, t < W <= 16 <= kGatherThreads
    if (tid < h) d[tid] = s[tid];
    if (tid < t) d[h + nv * W + tid] = s[h + nv * W + tid];
  }
}

// src_rows: rows of src; an index outside [0, src_rows) copies nothing (caller-supplied permutations)
__global__ __launch_bounds__(kGatherThreads) void k_carla_gather(const uint8_t* __restrict__ src,
                                                                 const int32_t* __restrict__ idx,
                                                                 uint8_t* __restrict__ dst, long n, long row_bytes,
                                                                 long chunks_per_row, long src_rows) {
  const long items = n * chunks_per_row;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long row = it / chunks_per_row, chunk = it - row * chunks_per_row;
    const long from = (long)idx[row];
    if (from < 0 || from >= src_rows) continue;
    const uint8_t* s = src + from * row_bytes;
    uint8_t* d = dst + row * row_bytes;
    const unsigned rel = (unsigned)((uintptr_t)s ^ (uintptr_t)d);
    if ((rel & 15u) == 0) gather_chunk<uint4>(s, d, row_bytes, chunk);
    else if ((rel & 3u) == 0) gather_chunk<uint32_t>(s, d, row_bytes, chunk);
    else gather_chunk<uint8_t>(s, d, row_bytes, chunk);
  }
}

int launch_gather(const void* src, const int32_t* idx, void* dst, long n, long row_bytes, long src_rows,
                  hipStream_t s) {
  if (n <= 0) return 0;
  const long cpr = (row_bytes + kGatherChunk - 1) / kGatherChunk;
  const long blocks = std::min<long>(n * cpr, kGatherMaxBlocks);
  hipLaunchKernelGGL(k_carla_gather, dim3((unsigned)blocks), dim3(kGatherThreads), 0, s, (const uint8_t*)src, idx,
                     (uint8_t*)dst, n, row_bytes, cpr, src_rows);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// The fp32 side arrays of a minibatch in one launch: segment k has rows of width[k] floats; one thread
// per (row, column of the concatenated widths). 17 floats per row for the default agent: the launch is
// latency, not bandwidth.
constexpr int kGatherMaxSeg = 8;
struct GatherF32Args {
  const float* src[kGatherMaxSeg];
  float* dst[kGatherMaxSeg];
  int width[kGatherMaxSeg];
  int nseg, total;  // total = sum of widths
  const int32_t* idx;
  long n, src_rows;
};
__global__ __launch_bounds__(256) void k_carla_gather_f32(GatherF32Args a) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n * a.total) return;
  const long row = g / a.total;
  int col = (int)(g - row * a.total);
  const long from = (long)a.idx[row];
  if (from < 0 || from >= a.src_rows) return;
#pragma unroll
  for (int k = 0; k < kGatherMaxSeg; ++k) {
    if (k >= a.nseg) break;
    if (col < a.width[k]) {
      a.dst[k][row * a.width[k] + col] = a.src[k][from * a.width[k] + col];
      return;
    }
    col -= a.width[k];
  }
}

int launch_gather_f32(GatherF32Args a, hipStream_t s) {
  a.total = 0;
  for (int k = 0; k < a.nseg; ++k) a.total += a.width[k];
  if (a.n <= 0 || a.total <= 0) return 0;
  const long threads = a.n * a.total;
  if ((threads + 255) / 256 > (long)INT_MAX) return -1;
  hipLaunchKernelGGL(k_carla_gather_f32, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// fin[0..6) = the last slot's loss statistics, fin[6] = the mean clipfrac over all slots (summed in
// step order, ac_ppo_carla.cpp:637), fin[7] = the last slot's gradient norm
__global__ void k_carla_rollout_fin(const float* __restrict__ slots, int nslots, float* __restrict__ fin) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float* last = slots + (long)(nslots - 1) * kCarlaStatSlot;
  for (int k = 0; k < 6; ++k) fin[k] = last[k];
  float sum = 0.0f;
  for (int i = 0; i < nslots; ++i) sum += slots[(long)i * kCarlaStatSlot + 5];
  fin[6] = sum / (float)nslots;
  fin[7] = last[6];
}

// losses/discounted_returns (ac_ppo_carla.cpp:626-658, :701): out[0] = mean over j < B of ret[j % Bc], the
// collected rows repeated and truncated to the full batch as the permutation is. One block, a fixed
// order: thread t adds its rows j = t, t + 256, ... in that order, then a tree over the 256 partial sums.
__global__ __launch_bounds__(256) void k_carla_returns_mean(const float* __restrict__ ret, long Bc, long B,
                                                            float* __restrict__ out) {
  __shared__ float red[256];
  float q = 0.f;
  for (long j = threadIdx.x; j < B; j += 256) q += ret[j % Bc];
  red[threadIdx.x] = q;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0] / (float)B;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------
struct ppo_carla_rollout {
  ppo_carla_t* agent = nullptr;
  ppo_carla_rollout_config cfg{};
  CarlaAgentInfo info{};
  int NM = 0, NV = 0, A = 0;
  long T = 0, E = 0, B = 0, M = 0;  // B = T E rows, M = B / num_minibatches
  long row_bytes = 0;               // C * IH * IW
  long iteration = 0;
  // storage [T, E, ...]
  uint8_t* bev = nullptr;
  float *meas = nullptr, *vmeas = nullptr, *actions = nullptr, *logp = nullptr, *rewards = nullptr, *dones = nullptr,
        *values = nullptr, *adv = nullptr, *ret = nullptr, *next_value = nullptr;
  // one minibatch, contiguous (what ppo_carla_update reads)
  uint8_t* mb_bev = nullptr;
  float *mb_meas = nullptr, *mb_vmeas = nullptr, *mb_actions = nullptr, *mb_logp = nullptr, *mb_adv = nullptr,
        *mb_ret = nullptr, *mb_values = nullptr;
  int32_t* perms = nullptr;  // [update_epochs][B]
  float* slots = nullptr;    // [update_epochs * num_minibatches][kCarlaStatSlot], then fin [8], then returns_mean [8]
  // act lanes (ppo_carla.h "act lanes"). lanes: created and destroyed under the exclusive flag only.
  // sync_ev: recorded after every gae / train; a lane's next act waits for it before it writes storage rows.
  ppo_carla_lane_t* lanes[PPO_CARLA_MAX_LANES] = {};
  hipEvent_t sync_ev = nullptr;
  std::atomic<int> lane_calls{0};  // lane calls inside the library
  std::atomic<int> exclusive{0};   // 1 while gae / train / lane_create / lane_destroy is inside the library
};

struct ppo_carla_lane {
  ppo_carla_rollout_t* r = nullptr;
  int slot = -1;  // index in r->lanes
  hipStream_t stream = nullptr;
  hipEvent_t ev = nullptr;  // after the last work queued on stream
  CarlaFwdBufs fb;          // one row
  uint8_t* pin = nullptr;   // pinned: bev row | action [A] | meas [NM] | vmeas [NV] | done | reward
  float* pin_f = nullptr;   // the floats of pin
};

namespace {

// Both guards are sequentially consistent counters: a lane call announces itself, then looks for an
// exclusive call; an exclusive call announces itself, then looks for lane calls. Whichever comes second
// sees the other, so of two calls that overlap at least one is refused.
struct LaneCallGuard {
  ppo_carla_rollout_t* r;
  bool ok;
  explicit LaneCallGuard(ppo_carla_rollout_t* r_) : r(r_) {
    r->lane_calls.fetch_add(1);
    ok = r->exclusive.load() == 0;
  }
  ~LaneCallGuard() { r->lane_calls.fetch_sub(1); }
};
struct ExclusiveGuard {
  ppo_carla_rollout_t* r;
  bool ok;
  explicit ExclusiveGuard(ppo_carla_rollout_t* r_) : r(r_) {
    ok = r->exclusive.exchange(1) == 0;
    if (ok && r->lane_calls.load() != 0) {
      r->exclusive.store(0);
      ok = false;
    }
  }
  ~ExclusiveGuard() {
    if (ok) r->exclusive.store(0);
  }
};

// the stream of a gae / train call waits for what every lane has queued
int r_wait_lanes(ppo_carla_rollout_t* r, hipStream_t s) {
  for (ppo_carla_lane_t* l : r->lanes)
    if (l && hipStreamWaitEvent(s, l->ev, 0) != hipSuccess) return -2;
  return 0;
}

// ------------------------------------------------------------------------------------------
// k_carla_lane_in: the small fp32 inputs of one act (or one reward) into their storage rows
// ------------------------------------------------------------------------------------------
// meas [NM], vmeas [NV], next_done and reward of one env are at most a few dozen floats: they travel in
// the kernel's argument block, and one wave writes them with one vector store per lane. That replaces
// three host-to-device copies of 32, 12 and 4 bytes per act (each a DMA submission) by one launch on
// the lane's stream. A NULL destination is skipped.
constexpr int kLaneInMax = 62;  // floats of meas + vmeas in the argument block (a 64-lane wave writes them)
struct LaneInArgs {
  float *meas, *vmeas, *done, *reward;  // destination rows
  int nm, nv;
  float done_v, reward_v;
  float v[kLaneInMax];  // meas, then vmeas
};
__global__ __launch_bounds__(64) void k_carla_lane_in(LaneInArgs a) {
  const int t = threadIdx.x;
  if (t < a.nm) a.meas[t] = a.v[t];
  else if (t < a.nm + a.nv && a.vmeas) a.vmeas[t - a.nm] = a.v[t];
  if (t == 62 && a.done) *a.done = a.done_v;
  if (t == 63 && a.reward) *a.reward = a.reward_v;
}

// host values -> rows on s. stage: host memory the copies of the wide path may read after the call
// returns (a lane's pinned buffer), nm + nv + 2 floats, or nullptr: the sources are read before return.
int lane_in(int nm, int nv, const float* meas, const float* vmeas, float done_v, float reward_v, float* meas_row,
            float* vmeas_row, float* done_row, float* reward_row, float* stage, hipStream_t s) {
  if (!vmeas_row) nv = 0;
  if (!meas_row) nm = 0;
  if (nm + nv <= kLaneInMax) {
    LaneInArgs a{};
    a.meas = meas_row; a.vmeas = vmeas_row; a.done = done_row; a.reward = reward_row;
    a.nm = nm; a.nv = nv; a.done_v = done_v; a.reward_v = reward_v;
    for (int i = 0; i < nm; ++i) a.v[i] = meas[i];
    for (int i = 0; i < nv; ++i) a.v[nm + i] = vmeas[i];
    hipLaunchKernelGGL(k_carla_lane_in, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
  }
  // wider than the argument block: one copy per array
  const size_t f = sizeof(float);
  float local[2] = {done_v, reward_v};
  const float *m = meas, *v = vmeas, *dr = local;
  if (stage) {
    if (nm) memcpy(stage, meas, nm * f);
    if (nv) memcpy(stage + nm, vmeas, nv * f);
    stage[nm + nv] = done_v;
    stage[nm + nv + 1] = reward_v;
    m = stage; v = stage + nm; dr = stage + nm + nv;
  }
  bool ok = true;
  if (nm) ok = ok && hipMemcpyAsync(meas_row, m, nm * f, hipMemcpyHostToDevice, s) == hipSuccess;
  if (nv) ok = ok && hipMemcpyAsync(vmeas_row, v, nv * f, hipMemcpyHostToDevice, s) == hipSuccess;
  if (done_row) ok = ok && hipMemcpyAsync(done_row, dr, f, hipMemcpyHostToDevice, s) == hipSuccess;
  if (reward_row) ok = ok && hipMemcpyAsync(reward_row, dr + 1, f, hipMemcpyHostToDevice, s) == hipSuccess;
  // without a staging buffer the sources are the caller's (or this frame's): they must have been read
  if (!stage) ok = ok && hipStreamSynchronize(s) == hipSuccess;
  return ok ? 0 : -2;
}

}  // namespace

static int r_alloc(void** p, size_t bytes) {
  if (hipMalloc(p, bytes ? bytes : 1) != hipSuccess) return -2;
  return hipMemset(*p, 0, bytes ? bytes : 1) == hipSuccess ? 0 : -2;
}

extern "C" int ppo_carla_rollout_destroy(ppo_carla_rollout_t* r) {
  if (!r) return 0;
  (void)hipSetDevice(r->info.device);
  if (r->info.stream) (void)hipStreamSynchronize(r->info.stream);
  void* bufs[] = {r->bev,    r->meas,    r->vmeas,     r->actions,  r->logp,   r->rewards, r->dones,
                  r->values, r->adv,     r->ret,       r->next_value, r->mb_bev, r->mb_meas, r->mb_vmeas,
                  r->mb_actions, r->mb_logp, r->mb_adv, r->mb_ret,  r->mb_values, r->perms, r->slots};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (r->sync_ev) (void)hipEventDestroy(r->sync_ev);
  for (ppo_carla_lane_t* l : r->lanes)  // a lane left behind: its handle dangles from here on
    if (l) l->r = nullptr;
  delete r;
  return 0;
}

extern "C" int ppo_carla_rollout_create(ppo_carla_t* agent, const ppo_carla_rollout_config* cfg,
                                        ppo_carla_rollout_t** out) {
  if (!agent || !cfg || !out) return ppo_fail("ppo_carla_rollout_create: null argument", -1);
  if (cfg->num_steps <= 0 || cfg->num_envs <= 0 || cfg->update_epochs <= 0 || cfg->num_minibatches <= 0)
    return ppo_fail("ppo_carla_rollout_create: num_steps, num_envs, update_epochs and num_minibatches must be positive",
                    -1);
  const long T = cfg->num_steps, E = cfg->num_envs, B = T * E;
  if (B >= (1L << 31)) return ppo_fail("ppo_carla_rollout_create: num_steps * num_envs must stay below 2^31", -1);
  if (B % cfg->num_minibatches != 0)
    return ppo_fail("ppo_carla_rollout_create: num_steps * num_envs = " + std::to_string(B) +
                    " is not divisible by num_minibatches = " + std::to_string(cfg->num_minibatches), -1);
  const long M = B / cfg->num_minibatches;
  CarlaAgentInfo info;
  if (int rc = carla_agent_info(agent, &info)) return rc;
  if ((long)info.max_batch < std::max(E, M))
    return ppo_fail("ppo_carla_rollout_create: the agent's max_batch " + std::to_string(info.max_batch) +
                    " is below max(num_envs, minibatch rows) = " + std::to_string(std::max(E, M)), -1);
  ppo_carla_layout2 L;
  if (int rc = ppo_carla_get_layout2(agent, &L)) return rc;
  if (hipSetDevice(info.device) != hipSuccess) return ppo_fail("ppo_carla_rollout_create: hipSetDevice failed", -2);
  ppo_carla_rollout_t* r = new ppo_carla_rollout_t();
  r->agent = agent;
  r->cfg = *cfg;
  r->info = info;
  r->NM = L.NM;
  r->NV = L.NV;
  r->A = L.A;
  r->T = T;
  r->E = E;
  r->B = B;
  r->M = M;
  r->row_bytes = (long)L.C * L.IH * L.IW;
  const size_t f = sizeof(float);
  const size_t uB = (size_t)B, uM = (size_t)M;
  const int nslots = cfg->update_epochs * cfg->num_minibatches;
  int bad = 0;
  bad |= r_alloc((void**)&r->bev, uB * (size_t)r->row_bytes);
  bad |= r_alloc((void**)&r->meas, uB * r->NM * f);
  bad |= r_alloc((void**)&r->vmeas, uB * r->NV * f);
  bad |= r_alloc((void**)&r->actions, uB * r->A * f);
  for (float** p : {&r->logp, &r->rewards, &r->dones, &r->values, &r->adv, &r->ret}) bad |= r_alloc((void**)p, uB * f);
  bad |= r_alloc((void**)&r->next_value, (size_t)E * f);
  bad |= r_alloc((void**)&r->mb_bev, uM * (size_t)r->row_bytes);
  bad |= r_alloc((void**)&r->mb_meas, uM * r->NM * f);
  bad |= r_alloc((void**)&r->mb_vmeas, uM * r->NV * f);
  bad |= r_alloc((void**)&r->mb_actions, uM * r->A * f);
  for (float** p : {&r->mb_logp, &r->mb_adv, &r->mb_ret, &r->mb_values}) bad |= r_alloc((void**)p, uM * f);
  bad |= r_alloc((void**)&r->perms, (size_t)cfg->update_epochs * uB * sizeof(int32_t));
  // the update slots, train's `fin` block, then ppo_carla_rollout_returns_mean's scalar
  bad |= r_alloc((void**)&r->slots, ((size_t)nslots + 2) * kCarlaStatSlot * f);
  bad |= hipEventCreateWithFlags(&r->sync_ev, hipEventDisableTiming) == hipSuccess ? 0 : 1;
  // the zero fills above ran on the null stream; the agent's stream does not wait for it
  if (!bad && hipDeviceSynchronize() != hipSuccess) bad = 1;
  if (bad) {
    ppo_carla_rollout_destroy(r);
    return ppo_fail("ppo_carla_rollout_create: device allocation failed", -2);
  }
  *out = r;
  return 0;
}

static hipStream_t r_stream(const ppo_carla_rollout_t* r, void* stream) {
  return stream ? (hipStream_t)stream : r->info.stream;
}

static int r_range(const ppo_carla_rollout_t* r, int step, int e0, int e1, const char* what) {
  if (step < 0 || step >= r->T) return ppo_fail(std::string(what) + ": step out of range", -1);
  if (e0 < 0 || e1 > r->E || e0 >= e1) return ppo_fail(std::string(what) + ": env range out of bounds", -1);
  return 0;
}

extern "C" int ppo_carla_rollout_act(ppo_carla_rollout_t* r, int step, int env_begin, int env_end, const uint8_t* bev,
                                     const float* meas, const float* vmeas, const float* next_done, float* action_out,
                                     void* stream) {
  if (!r || !bev || !meas || !next_done || (!vmeas && r->NV > 0))
    return ppo_fail("ppo_carla_rollout_act: null argument", -1);
  if (int rc = r_range(r, step, env_begin, env_end, "ppo_carla_rollout_act")) return rc;
  if (hipSetDevice(r->info.device) != hipSuccess) return ppo_fail("ppo_carla_rollout_act: hipSetDevice failed", -2);
  hipStream_t s = r_stream(r, stream);
  const long row = (long)step * r->E + env_begin;
  const size_t n = (size_t)(env_end - env_begin), f = sizeof(float);
  uint8_t* s_bev = r->bev + row * r->row_bytes;
  float* s_meas = r->meas + row * r->NM;
  float* s_vmeas = r->vmeas + row * r->NV;
  // :365-368 the observation and done rows of this step
  bool ok = hipMemcpyAsync(s_bev, bev, n * (size_t)r->row_bytes, hipMemcpyDeviceToDevice, s) == hipSuccess;
  ok = ok && hipMemcpyAsync(s_meas, meas, n * r->NM * f, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (r->NV > 0) ok = ok && hipMemcpyAsync(s_vmeas, vmeas, n * r->NV * f, hipMemcpyDeviceToDevice, s) == hipSuccess;
  ok = ok && hipMemcpyAsync(r->dones + row, next_done, n * f, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (!ok) return ppo_fail("ppo_carla_rollout_act: copy failed", -2);
  // :372-379 sample on the stored rows; action, log-prob and value go straight into the storage
  float* s_act = r->actions + row * r->A;
  int rc = ppo_carla_forward(r->agent, (int)n, s_bev, s_meas, r->NV > 0 ? s_vmeas : nullptr, PPO_CARLA_SAMPLE, nullptr,
                             env_begin, r->iteration * r->T + step, s_act, r->logp + row, nullptr, r->values + row,
                             nullptr, nullptr, s);
  if (rc) return rc;
  if (action_out && hipMemcpyAsync(action_out, s_act, n * r->A * f, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return ppo_fail("ppo_carla_rollout_act: copy failed", -2);
  return 0;
}

extern "C" int ppo_carla_rollout_reward(ppo_carla_rollout_t* r, int step, int env_begin, int env_end,
                                        const float* reward, void* stream) {
  if (!r || !reward) return ppo_fail("ppo_carla_rollout_reward: null argument", -1);
  if (int rc = r_range(r, step, env_begin, env_end, "ppo_carla_rollout_reward")) return rc;
  if (hipSetDevice(r->info.device) != hipSuccess) return ppo_fail("ppo_carla_rollout_reward: hipSetDevice failed", -2);
  if (hipMemcpyAsync(r->rewards + (long)step * r->E + env_begin, reward, (size_t)(env_end - env_begin) * sizeof(float),
                     hipMemcpyDeviceToDevice, r_stream(r, stream)) != hipSuccess)
    return ppo_fail("ppo_carla_rollout_reward: copy failed", -2);
  return 0;
}

extern "C" int ppo_carla_rollout_gae(ppo_carla_rollout_t* r, const uint8_t* next_bev, const float* next_meas,
                                     const float* next_vmeas, const float* next_done, int num_steps_collected,
                                     void* stream) {
  if (!r || !next_bev || !next_meas || !next_done || (!next_vmeas && r->NV > 0))
    return ppo_fail("ppo_carla_rollout_gae: null argument", -1);
  if (num_steps_collected <= 0 || num_steps_collected > r->T)
    return ppo_fail("ppo_carla_rollout_gae: bad collected step count", -1);
  ExclusiveGuard guard(r);
  if (!guard.ok) return ppo_fail("ppo_carla_rollout_gae: called while a lane call is inside the library", -1);
  if (hipSetDevice(r->info.device) != hipSuccess) return ppo_fail("ppo_carla_rollout_gae: hipSetDevice failed", -2);
  hipStream_t s = r_stream(r, stream);
  if (r_wait_lanes(r, s)) return ppo_fail("ppo_carla_rollout_gae: waiting for the lanes failed", -2);
  // :486 get_value on the next observation
  int rc = ppo_carla_forward(r->agent, (int)r->E, next_bev, next_meas, next_vmeas, PPO_CARLA_MEAN, nullptr, 0, 0,
                             nullptr, nullptr, nullptr, r->next_value, nullptr, nullptr, s);
  if (rc) return rc;
  GaeArgs g;
  g.rewards = r->rewards;
  g.values = r->values;
  g.dones = r->dones;
  g.next_value = r->next_value;
  g.next_done = next_done;
  // a partial collection bootstraps from the stored step num_steps_collected (ppo_carla.h, :490-498)
  if (num_steps_collected < r->T) {
    g.next_value = r->values + (long)num_steps_collected * r->E;
    g.next_done = r->dones + (long)num_steps_collected * r->E;
  }
  g.adv = r->adv;
  g.ret = r->ret;
  g.T = num_steps_collected;
  g.E = (int)r->E;
  g.gamma = r->cfg.gamma;
  g.lam = r->cfg.gae_lambda;
  launch_gae(g, s);  // writes returns = advantages + values with the advantages (:503)
  if (hipGetLastError() != hipSuccess) return ppo_fail("ppo_carla_rollout_gae: launch failed", -2);
  if (hipEventRecord(r->sync_ev, s) != hipSuccess) return ppo_fail("ppo_carla_rollout_gae: hipEventRecord failed", -2);
  return 0;
}

extern "C" int ppo_carla_rollout_train(ppo_carla_rollout_t* r, const ppo_carla_train_config* tc, float lr,
                                       int num_steps_collected, const int32_t* perms_dev, ppo_carla_update_stats* last,
                                       float* mean_clipfrac) {
  if (!r || !tc) return ppo_fail("ppo_carla_rollout_train: null argument", -1);
  if (num_steps_collected <= 0 || num_steps_collected > r->T)
    return ppo_fail("ppo_carla_rollout_train: bad collected step count", -1);
  ExclusiveGuard guard(r);
  if (!guard.ok) return ppo_fail("ppo_carla_rollout_train: called while a lane call is inside the library", -1);
  if (hipSetDevice(r->info.device) != hipSuccess) return ppo_fail("ppo_carla_rollout_train: hipSetDevice failed", -2);
  hipStream_t s = r->info.stream;
  if (r_wait_lanes(r, s)) return ppo_fail("ppo_carla_rollout_train: waiting for the lanes failed", -2);
  const int EP = r->cfg.update_epochs, MB = r->cfg.num_minibatches;
  const long B = r->B, M = r->M, Bc = (long)num_steps_collected * r->E;
  // ---- permutations (:532-538), as ppo_update_ex ----
  if (perms_dev) {
    if (hipMemcpyAsync(r->perms, perms_dev, sizeof(int32_t) * (size_t)EP * B, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return ppo_fail("ppo_carla_rollout_train: copy failed", -2);
  } else {
    for (int e = 0; e < EP; ++e) {
      int32_t* dst = r->perms + (size_t)e * B;
      launch_perm(dst, (uint32_t)Bc, make_perm_key(r->cfg.seed, r->cfg.rank, r->iteration * (long)EP + e, Bc), s);
      for (long have = Bc; have < B;) {  // doubling copies of the periodic prefix
        const long n = std::min(have, B - have);
        if (hipMemcpyAsync(dst + have, dst, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, s) != hipSuccess)
          return ppo_fail("ppo_carla_rollout_train: copy failed", -2);
        have += n;
      }
    }
  }
  // ---- epochs x minibatches (:531-620) ----
  GatherF32Args ga{};
  const float* srcs[] = {r->meas, r->vmeas, r->actions, r->logp, r->adv, r->ret, r->values};
  float* dsts[] = {r->mb_meas, r->mb_vmeas, r->mb_actions, r->mb_logp, r->mb_adv, r->mb_ret, r->mb_values};
  const int widths[] = {r->NM, r->NV, r->A, 1, 1, 1, 1};
  ga.nseg = 7;
  for (int k = 0; k < 7; ++k) {
    ga.src[k] = srcs[k];
    ga.dst[k] = dsts[k];
    ga.width[k] = widths[k];
  }
  ga.n = M;
  ga.src_rows = B;
  for (int e = 0; e < EP; ++e)
    for (int mb = 0; mb < MB; ++mb) {
      const int32_t* idx = r->perms + (size_t)e * B + (size_t)mb * M;
      ga.idx = idx;
      if (launch_gather(r->bev, idx, r->mb_bev, M, r->row_bytes, B, s) != 0 || launch_gather_f32(ga, s) != 0)
        return ppo_fail("ppo_carla_rollout_train: gather launch failed", -2);
      int rc = ppo_carla_update(r->agent, tc, (int)M, r->mb_bev, r->mb_meas, r->NV > 0 ? r->mb_vmeas : nullptr,
                                r->mb_actions, r->mb_logp, r->mb_adv, r->mb_ret, r->mb_values, lr, nullptr, s);
      if (rc) return rc;
      rc = carla_stats_to_slot(r->agent, r->slots + (size_t)(e * MB + mb) * kCarlaStatSlot, s);
      if (rc) return rc;
    }
  r->iteration += 1;
  // the gathers above read the storage rows a lane's next act overwrites
  if (hipEventRecord(r->sync_ev, s) != hipSuccess) return ppo_fail("ppo_carla_rollout_train: hipEventRecord failed", -2);
  if (last || mean_clipfrac) {
    const int nslots = EP * MB;
    float* fin = r->slots + (size_t)nslots * kCarlaStatSlot;
    hipLaunchKernelGGL(k_carla_rollout_fin, dim3(1), dim3(64), 0, s, r->slots, nslots, fin);
    if (hipGetLastError() != hipSuccess) return ppo_fail("ppo_carla_rollout_train: launch failed", -2);
    // :645-651 the logged values are rank averages (the gradient norm is global already)
    if (int rc = ppo_carla_comm_allreduce(r->agent, fin, 7, 1)) return rc;
    float h[8];
    if (hipMemcpyAsync(h, fin, sizeof h, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return ppo_fail("ppo_carla_rollout_train: stats copy failed", -2);
    if (last) {
      last->pg_loss = h[0];
      last->v_loss = h[1];
      last->entropy = h[2];
      last->old_approx_kl = h[3];
      last->approx_kl = h[4];
      last->clipfrac = h[5];
      last->grad_norm = h[7];
    }
    if (mean_clipfrac) *mean_clipfrac = h[6];
  }
  return 0;
}

extern "C" int ppo_carla_rollout_returns_mean(ppo_carla_rollout_t* r, int num_steps_collected, float* out) {
  if (!r || !out) return ppo_fail("ppo_carla_rollout_returns_mean: null argument", -1);
  if (num_steps_collected <= 0 || num_steps_collected > r->T)
    return ppo_fail("ppo_carla_rollout_returns_mean: bad collected step count", -1);
  ExclusiveGuard guard(r);
  if (!guard.ok) return ppo_fail("ppo_carla_rollout_returns_mean: called while a lane call is inside the library", -1);
  if (hipSetDevice(r->info.device) != hipSuccess)
    return ppo_fail("ppo_carla_rollout_returns_mean: hipSetDevice failed", -2);
  hipStream_t s = r->info.stream;
  // the slot after train's `fin` block is free between calls: calls on one object are serial
  float* slot = r->slots + ((size_t)r->cfg.update_epochs * r->cfg.num_minibatches + 1) * kCarlaStatSlot;
  hipLaunchKernelGGL(k_carla_returns_mean, dim3(1), dim3(256), 0, s, r->ret, (long)num_steps_collected * r->E, r->B,
                     slot);
  if (hipGetLastError() != hipSuccess) return ppo_fail("ppo_carla_rollout_returns_mean: launch failed", -2);
  if (int rc = ppo_carla_comm_allreduce(r->agent, slot, 1, 1)) return rc;  // :650 averaged over ranks
  if (hipMemcpyAsync(out, slot, sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return ppo_fail("ppo_carla_rollout_returns_mean: copy failed", -2);
  return 0;
}

extern "C" int ppo_carla_rollout_buffer(ppo_carla_rollout_t* r, int which, void** dev_ptr) {
  if (!r || !dev_ptr) return ppo_fail("ppo_carla_rollout_buffer: null argument", -1);
  void* p[PPO_CARLA_BUF_COUNT] = {r->bev,     r->meas,  r->vmeas,  r->actions, r->logp,      r->rewards,
                                  r->dones,   r->values, r->adv,   r->ret,     r->next_value};
  if (which < 0 || which >= PPO_CARLA_BUF_COUNT) return ppo_fail("ppo_carla_rollout_buffer: unknown buffer", -1);
  *dev_ptr = p[which];
  return 0;
}

extern "C" int ppo_carla_rollout_last_perms(ppo_carla_rollout_t* r, int32_t* host, long n) {
  if (!r || !host) return ppo_fail("ppo_carla_rollout_last_perms: null argument", -1);
  const long want = (long)r->cfg.update_epochs * r->B;
  if (n != want) return ppo_fail("ppo_carla_rollout_last_perms: expected " + std::to_string(want) + " indices", -1);
  if (hipSetDevice(r->info.device) != hipSuccess || hipStreamSynchronize(r->info.stream) != hipSuccess ||
      hipMemcpy(host, r->perms, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
    return ppo_fail("ppo_carla_rollout_last_perms: copy failed", -2);
  return 0;
}

extern "C" long ppo_carla_rollout_iteration(const ppo_carla_rollout_t* r) { return r ? r->iteration : -1; }

extern "C" int ppo_carla_rollout_set_iteration(ppo_carla_rollout_t* r, long iteration) {
  if (!r || iteration < 0) return ppo_fail("ppo_carla_rollout_set_iteration: bad argument", -1);
  r->iteration = iteration;
  return 0;
}

// ------------------------------------------------------------------------------------------
// act lanes (ppo_carla.h "act lanes"): ac_ppo_carla.cpp:355-417, one thread / stream / forward per env
// ------------------------------------------------------------------------------------------
static void lane_free(ppo_carla_lane_t* l) {
  carla_fwd_free(&l->fb);
  if (l->pin) (void)hipHostFree(l->pin);
  if (l->ev) (void)hipEventDestroy(l->ev);
  if (l->stream) (void)hipStreamDestroy(l->stream);
  delete l;
}

extern "C" int ppo_carla_lane_create(ppo_carla_rollout_t* r, ppo_carla_lane_t** out) {
  if (!r || !out) return ppo_fail("ppo_carla_lane_create: null argument", -1);
  ExclusiveGuard guard(r);
  if (!guard.ok) return ppo_fail("ppo_carla_lane_create: called while another call on the object is inside the library", -1);
  int slot = 0;
  while (slot < PPO_CARLA_MAX_LANES && r->lanes[slot]) ++slot;
  if (slot == PPO_CARLA_MAX_LANES)
    return ppo_fail("ppo_carla_lane_create: a rollout object has at most " + std::to_string(PPO_CARLA_MAX_LANES) +
                    " lanes", -1);
  if (hipSetDevice(r->info.device) != hipSuccess) return ppo_fail("ppo_carla_lane_create: hipSetDevice failed", -2);
  ppo_carla_lane_t* l = new ppo_carla_lane_t();
  l->r = r;
  l->slot = slot;
  // bev row, padded to whole floats, then action | meas | vmeas | done | reward
  const size_t bev_pad = ((size_t)r->row_bytes + 15) & ~(size_t)15;
  const size_t nfl = (size_t)r->A + r->NM + r->NV + 2;
  bool ok = hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&l->ev, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&l->pin, bev_pad + nfl * sizeof(float), hipHostMallocDefault) == hipSuccess;
  ok = ok && carla_fwd_alloc(r->agent, 1, &l->fb) == 0;
  // the zero fills of the buffers ran on the null stream; the lane's stream does not wait for it
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    lane_free(l);
    return ppo_fail("ppo_carla_lane_create: allocation failed", -2);
  }
  l->pin_f = reinterpret_cast<float*>(l->pin + bev_pad);
  r->lanes[slot] = l;
  *out = l;
  return 0;
}

extern "C" int ppo_carla_lane_destroy(ppo_carla_lane_t* l) {
  if (!l) return 0;
  ppo_carla_rollout_t* r = l->r;
  if (r) {
    ExclusiveGuard guard(r);
    if (!guard.ok)
      return ppo_fail("ppo_carla_lane_destroy: called while another call on the object is inside the library", -1);
    (void)hipSetDevice(r->info.device);
    (void)hipStreamSynchronize(l->stream);
    r->lanes[l->slot] = nullptr;
    lane_free(l);
    return 0;
  }
  (void)hipStreamSynchronize(l->stream);  // the rollout object went first
  lane_free(l);
  return 0;
}

// the checks every lane call starts with, none of which needs the device
static int lane_check(const ppo_carla_lane_t* l, int step, int env, const char* what) {
  if (!l->r) return ppo_fail(std::string(what) + ": the lane's rollout object was destroyed", -1);
  if (step < 0 || step >= l->r->T) return ppo_fail(std::string(what) + ": step out of range", -1);
  if (env < 0 || env >= l->r->E) return ppo_fail(std::string(what) + ": env out of range", -1);
  return 0;
}

extern "C" int ppo_carla_lane_act(ppo_carla_lane_t* l, int step, int env, const uint8_t* bev, const float* meas,
                                  const float* vmeas, float next_done, float* action_host) {
  if (!l || !bev || !meas || !action_host || (l->r && !vmeas && l->r->NV > 0))
    return ppo_fail("ppo_carla_lane_act: null argument", -1);
  if (int rc = lane_check(l, step, env, "ppo_carla_lane_act")) return rc;
  ppo_carla_rollout_t* r = l->r;
  LaneCallGuard guard(r);
  if (!guard.ok) return ppo_fail("ppo_carla_lane_act: called while gae, train or a lane's creation is inside the library", -1);
  if (hipSetDevice(r->info.device) != hipSuccess) return ppo_fail("ppo_carla_lane_act: hipSetDevice failed", -2);
  hipStream_t s = l->stream;
  // the parameters of the last update / load, and the last gae / train's reads of the storage
  if (int rc = carla_params_wait(r->agent, s)) return rc;
  if (hipStreamWaitEvent(s, r->sync_ev, 0) != hipSuccess) return ppo_fail("ppo_carla_lane_act: hipStreamWaitEvent failed", -2);
  const long row = (long)step * r->E + env;
  uint8_t* s_bev = r->bev + row * r->row_bytes;
  float* s_meas = r->meas + row * r->NM;
  float* s_vmeas = r->NV > 0 ? r->vmeas + row * r->NV : nullptr;
  float* s_act = r->actions + row * r->A;
  // :365-368 the observation row: pinned buffer (free: the previous act ended with a wait on s), one DMA
  memcpy(l->pin, bev, (size_t)r->row_bytes);
  if (hipMemcpyAsync(s_bev, l->pin, (size_t)r->row_bytes, hipMemcpyHostToDevice, s) != hipSuccess)
    return ppo_fail("ppo_carla_lane_act: copy failed", -2);
  if (lane_in(r->NM, r->NV, meas, vmeas, next_done, 0.0f, s_meas, s_vmeas, r->dones + row, nullptr, l->pin_f + r->A, s))
    return ppo_fail("ppo_carla_lane_act: storing the measurements failed", -2);
  // :372-379 sample on the stored row with the keys of ppo_carla_rollout_act(step, env, env + 1)
  if (int rc = carla_forward(r->agent, l->fb, s, 1, s_bev, s_meas, s_vmeas, PPO_CARLA_SAMPLE, nullptr, env,
                             r->iteration * r->T + step, s_act, r->logp + row, nullptr, r->values + row, nullptr,
                             nullptr))
    return rc;
  if (hipMemcpyAsync(l->pin_f, s_act, (size_t)r->A * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipEventRecord(l->ev, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return ppo_fail("ppo_carla_lane_act: reading the action back failed", -2);
  memcpy(action_host, l->pin_f, (size_t)r->A * sizeof(float));
  return 0;
}

extern "C" int ppo_carla_lane_reward(ppo_carla_lane_t* l, int step, int env, float reward) {
  if (!l) return ppo_fail("ppo_carla_lane_reward: null argument", -1);
  if (int rc = lane_check(l, step, env, "ppo_carla_lane_reward")) return rc;
  ppo_carla_rollout_t* r = l->r;
  LaneCallGuard guard(r);
  if (!guard.ok)
    return ppo_fail("ppo_carla_lane_reward: called while gae, train or a lane's creation is inside the library", -1);
  if (hipSetDevice(r->info.device) != hipSuccess) return ppo_fail("ppo_carla_lane_reward: hipSetDevice failed", -2);
  // always within the argument block: nothing is staged
  if (lane_in(0, 0, nullptr, nullptr, 0.0f, reward, nullptr, nullptr, nullptr, r->rewards + (long)step * r->E + env,
              nullptr, l->stream) ||
      hipEventRecord(l->ev, l->stream) != hipSuccess)
    return ppo_fail("ppo_carla_lane_reward: launch failed", -2);
  return 0;
}

extern "C" int ppo_carla_lane_sync(ppo_carla_lane_t* l) {
  if (!l) return ppo_fail("ppo_carla_lane_sync: null argument", -1);
  if (!l->r) return ppo_fail("ppo_carla_lane_sync: the lane's rollout object was destroyed", -1);
  LaneCallGuard guard(l->r);
  if (!guard.ok) return ppo_fail("ppo_carla_lane_sync: called while gae, train or a lane's creation is inside the library", -1);
  if (hipSetDevice(l->r->info.device) != hipSuccess || hipStreamSynchronize(l->stream) != hipSuccess)
    return ppo_fail("ppo_carla_lane_sync: synchronisation failed", -2);
  return 0;
}

// ------------------------------------------------------------------------------------------
// test hooks (ppo_carla.h)
// ------------------------------------------------------------------------------------------
extern "C" int ppo_carla_debug_lane_in(int nm, int nv, const float* meas, const float* vmeas, float next_done,
                                       float reward, float* meas_row, float* vmeas_row, float* done_row,
                                       float* reward_row, void* stream) {
  if (nm < 0 || nv < 0) return ppo_fail("ppo_carla_debug_lane_in: nm and nv must be >= 0", -1);
  if ((nm > 0 && (!meas || !meas_row)) || (nv > 0 && (!vmeas || !vmeas_row)))
    return ppo_fail("ppo_carla_debug_lane_in: null argument", -1);
  if (int rc = ppo_runtime_check()) return rc;
  if (lane_in(nm, nv, meas, vmeas, next_done, reward, nm ? meas_row : nullptr, nv ? vmeas_row : nullptr, done_row,
              reward_row, nullptr, (hipStream_t)stream) != 0 ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return ppo_fail("ppo_carla_debug_lane_in: launch failed", -2);
  return 0;
}

extern "C" int ppo_carla_debug_gather(long n, long row_bytes, const void* src, const int32_t* idx, void* dst,
                                      void* stream) {
  if (!src || !idx || !dst) return ppo_fail("ppo_carla_debug_gather: null argument", -1);
  if (n < 0 || row_bytes <= 0) return ppo_fail("ppo_carla_debug_gather: n must be >= 0 and row_bytes positive", -1);
  if (n == 0) return 0;
  if (int rc = ppo_runtime_check()) return rc;
  if (launch_gather(src, idx, dst, n, row_bytes, LONG_MAX / row_bytes, (hipStream_t)stream) != 0 ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return ppo_fail("ppo_carla_debug_gather: launch failed", -2);
  return 0;
}

extern "C" int ppo_carla_debug_gather_f32(long n, int nseg, const float* const* src, const int* width,
                                          const int32_t* idx, float* const* dst, void* stream) {
  if (!src || !width || !idx || !dst) return ppo_fail("ppo_carla_debug_gather_f32: null argument", -1);
  if (n < 0 || nseg <= 0 || nseg > kGatherMaxSeg)
    return ppo_fail("ppo_carla_debug_gather_f32: n must be >= 0 and nseg in [1, 8]", -1);
  GatherF32Args a{};
  a.nseg = nseg;
  for (int k = 0; k < nseg; ++k) {
    if (!src[k] || !dst[k] || width[k] < 0) return ppo_fail("ppo_carla_debug_gather_f32: bad segment", -1);
    a.src[k] = src[k];
    a.dst[k] = dst[k];
    a.width[k] = width[k];
  }
  if (n == 0) return 0;
  a.idx = idx;
  a.n = n;
  a.src_rows = LONG_MAX;
  if (int rc = ppo_runtime_check()) return rc;
  if (launch_gather_f32(a, (hipStream_t)stream) != 0 || hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return ppo_fail("ppo_carla_debug_gather_f32: launch failed", -2);
  return 0;
}
