// ppo_capi_comm.hip — the data-parallel communicator of a context: RCCL (ppo_comm_init), which replaces
// torchfort::Comm (reference src/distributed.cpp), or the caller's host transport (ppo_comm_init_host),
// and the in-place all-reduce the update runs over either.
#include "ppo_capi_internal.hpp"

// In-place all-reduce over the attached communicator (no communicator: identity). RCCL runs on the
// context stream; the host transport synchronises the stream, hands the values to the caller's
// function in host memory and copies the result back.
int allreduce(ppo_t* c, float* buf, long n, int average, hipStream_t s) {
  if (c->comm) {
    ProfScope ps(c, PK_ALLREDUCE, s);
    NCCL_TRY(ncclAllReduce(buf, buf, (size_t)n, ncclFloat, average ? ncclAvg : ncclSum, c->comm, s));
    return 0;
  }
  if (c->host_ar) {
    if ((long)c->host_stage.size() < n) c->host_stage.resize((size_t)n);
    float* h = c->host_stage.data();
    HIP_TRY(hipMemcpyAsync(h, buf, sizeof(float) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (c->host_ar(h, n, average, c->host_user) != 0) return fail("ppo host all-reduce callback failed", -3);
    HIP_TRY(hipMemcpyAsync(buf, h, sizeof(float) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // the staging buffer is reused by the next call
  }
  return 0;
}

extern "C" int ppo_comm_unique_id(char id_out[PPO_COMM_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) <= PPO_COMM_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  memset(id_out, 0, PPO_COMM_ID_BYTES);
  memcpy(id_out, &id, sizeof(id));
  return 0;
}

void comm_detach(ppo_t* c) {
  if (c->comm) (void)ncclCommDestroy(c->comm);
  c->comm = nullptr;
  c->host_ar = nullptr;
  c->host_user = nullptr;
  c->world = 1;
}

// A real RCCL communicator for every world size, world = 1 included: a one-rank group runs the
// same distributed update sequence (advantage statistics, gradient and stats all-reduces) as a
// multi-GPU job, which is how the single-GPU tests exercise it.
extern "C" int ppo_comm_init(ppo_t* c, const char id[PPO_COMM_ID_BYTES], int rank, int world) {
  if (!c || !id) return fail("ppo_comm_init: null argument");
  if (world < 1 || rank < 0 || rank >= world) return fail("ppo_comm_init: bad rank / world size");
  HIP_TRY(hipSetDevice(c->device));
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));
  comm_detach(c);
  NCCL_TRY(ncclCommInitRank(&c->comm, world, uid, rank));
  c->rank = rank;
  c->world = world;
  return 0;
}

extern "C" int ppo_comm_init_host(ppo_t* c, int rank, int world, ppo_host_allreduce_fn fn, void* user) {
  if (!c || !fn) return fail("ppo_comm_init_host: null argument");
  if (world < 1 || rank < 0 || rank >= world) return fail("ppo_comm_init_host: bad rank / world size");
  comm_detach(c);
  c->host_ar = fn;
  c->host_user = user;
  c->rank = rank;
  c->world = world;
  return 0;
}

extern "C" int ppo_comm_destroy(ppo_t* c) {
  if (!c) return fail("null ctx");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  comm_detach(c);
  return 0;
}

extern "C" int ppo_comm_broadcast_params(ppo_t* c, int root) {
  if (!c) return fail("null ctx");
  if (!distributed(c)) return 0;
  if (root < 0 || root >= c->world) return fail("ppo_comm_broadcast_params: bad root");
  HIP_TRY(hipSetDevice(c->device));
  if (c->comm) {
    NCCL_TRY(ncclBroadcast(c->P, c->P, (size_t)c->K.size, ncclFloat, root, c->comm, c->stream));
  } else {  // host transport: sum with zeros from every rank but the root (x + 0 == x exactly)
    if (c->rank != root) HIP_TRY(hipMemsetAsync(c->P, 0, sizeof(float) * c->K.size, c->stream));
    if (allreduce(c, c->P, (long)c->K.size, 0, c->stream)) return -3;
  }
  if (refresh_weight_copies(c)) return -2;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int ppo_comm_allreduce(ppo_t* c, float* buf, long n, int average) {
  if (!c || !buf) return fail("null argument");
  return allreduce(c, buf, n, average, c->stream);
}

extern "C" int ppo_comm_info(const ppo_t* c, int* kind, int* rank, int* world) {
  if (!c || !kind || !rank || !world) return fail("ppo_comm_info: null argument");
  if (c->comm) {
    *kind = PPO_COMM_RCCL;
    NCCL_TRY(ncclCommCount(c->comm, world));
    NCCL_TRY(ncclCommUserRank(c->comm, rank));
  } else if (c->host_ar) {
    *kind = PPO_COMM_HOST;
    *rank = c->rank;
    *world = c->world;
  } else {
    *kind = PPO_COMM_NONE;
    *rank = c->rank;
    *world = c->world;
  }
  return 0;
}
