// krcn_comm.hip — the RCCL communicator and the virtual communicator (P ranks
// on one device).
#include "krcn_internal.hpp"

using namespace krcn;

// ------------------------------------------------------------- comm
extern "C" krcn_status krcn_comm_unique_id(void* uid128_host) {
  if (!uid128_host) return fail(KRCN_ERR_INVALID, "krcn_comm_unique_id: null argument");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  std::memcpy(uid128_host, &id, sizeof(id));
  return KRCN_OK;
}

extern "C" krcn_status krcn_comm_create(int nranks, int rank, const void* uid128_host, int device,
                                        krcn_comm** out) {
  if (!out || !uid128_host) return fail(KRCN_ERR_INVALID, "krcn_comm_create: null argument");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(KRCN_ERR_INVALID, "krcn_comm_create: bad rank %d of %d", rank, nranks);
  HIPCHK(hipSetDevice(device));
  ncclUniqueId id;
  std::memcpy(&id, uid128_host, sizeof(id));
  krcn_comm* c = new krcn_comm();
  c->nranks = nranks;
  c->rank = rank;
  c->device = device;
  ncclResult_t r = ncclCommInitRank(&c->comm, nranks, id, rank);
  if (r != ncclSuccess) {
    delete c;
    return fail(KRCN_ERR_RCCL, "ncclCommInitRank -> %s", ncclGetErrorString(r));
  }
  *out = c;
  return KRCN_OK;
}

// ------------------------------------------------- virtual communicator
// P ranks on ONE device, one host thread each (SURVEY.md §4 "P virtual shards
// on 1 GPU"): the partition, the rank-level plans and every sharded kernel
// run exactly as in a P-GPU job; only the collective differs — a rendezvous
// of the rank threads and a device sum in rank order stand in for RCCL's
// all-reduce (RCCL refuses two ranks on one device).
struct VirtualGroup : krcn::Rendezvous {
  int device = 0;
};

template <typename T>
__global__ __launch_bounds__(kNT) void k_virtual_sum(int P, int64_t count, VirtualBufs b) {
  for (int64_t i = int64_t(blockIdx.x) * kNT + threadIdx.x; i < count; i += int64_t(gridDim.x) * kNT) {
    T s = static_cast<const T*>(b.p[0])[i];
    for (int r = 1; r < P; ++r) s = s + static_cast<const T*>(b.p[r])[i];
    for (int r = 0; r < P; ++r) static_cast<T*>(b.p[r])[i] = s;
  }
}

krcn_status virtual_allreduce(krcn_comm* c, void* buf, int64_t count, int dtype, hipStream_t s) {
  HIPCHK(hipStreamSynchronize(s));   // this rank's buffer is final
  // the last to arrive sums every rank's buffer in rank order on its own stream
  auto sum = [s](void* const* bufs, int P, int64_t cnt, int dt) -> int {
    VirtualBufs vb{};
    for (int r = 0; r < P; ++r) vb.p[r] = bufs[r];
    const int grid = vec_grid(cnt);
    if (dt == KRCN_F64)
      hipLaunchKernelGGL(k_virtual_sum<double>, dim3(grid), dim3(kNT), 0, s, P, cnt, vb);
    else
      hipLaunchKernelGGL(k_virtual_sum<float>, dim3(grid), dim3(kNT), 0, s, P, cnt, vb);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e == hipSuccess ? KRCN_OK : KRCN_ERR_HIP;
  };
  std::string msg;
  const int r = c->vg->arrive(c->rank, &c->seq, buf, count, dtype, sum, &msg);
  if (r != KRCN_OK) return fail(r, "%s", msg.c_str());
  return KRCN_OK;
}

extern "C" krcn_status krcn_comm_create_virtual(int nranks, int device, krcn_comm** out) {
  if (!out) return fail(KRCN_ERR_INVALID, "krcn_comm_create_virtual: null argument");
  if (nranks < 1 || nranks > kVirtualMaxRanks)
    return fail(KRCN_ERR_INVALID, "krcn_comm_create_virtual: nranks must be 1..%d", kVirtualMaxRanks);
  HIPCHK(hipSetDevice(device));
  VirtualGroup* g = new VirtualGroup();
  g->P = nranks;
  g->device = device;
  g->alive = nranks;
  g->timeout_s = kVirtualTimeoutS;
  for (int r = 0; r < nranks; ++r) {
    krcn_comm* c = new krcn_comm();
    c->nranks = nranks;
    c->rank = r;
    c->device = device;
    c->vg = g;
    out[r] = c;
  }
  return KRCN_OK;
}

extern "C" krcn_status krcn_comm_destroy(krcn_comm* c) {
  if (!c) return KRCN_OK;
  if (c->comm) ncclCommDestroy(c->comm);
  if (c->vg) {
    bool last;
    {
      std::lock_guard<std::mutex> lk(c->vg->mu);
      last = --c->vg->alive == 0;
    }
    if (last) delete c->vg;
  }
  delete c;
  return KRCN_OK;
}

extern "C" krcn_status krcn_comm_allreduce(krcn_comm* c, int dtype, void* buf, int64_t n, void* stream) {
  if (!c || (!buf && n)) return fail(KRCN_ERR_INVALID, "krcn_comm_allreduce: null argument");
  if (n == 0 || c->nranks == 1) return KRCN_OK;
  HIPCHK(hipSetDevice(c->device));
  if (c->vg) return virtual_allreduce(c, buf, n, dtype, S(stream));
  ncclDataType_t t;
  nccl_dtype(dtype, &t);
  NCCLCHK(ncclAllReduce(buf, buf, size_t(n), t, ncclSum, c->comm, S(stream)));
  return KRCN_OK;
}
