// Host layer, part 4: RCCL as the exchange of the sharded pass (uglad_glad_forward_sharded): resolved at run time from the RCCL that is
// already in the process (PyTorch-ROCm's) or, failing that, the system's -- libuglad_hip.so itself has no link-time dependency on it.
#pragma once
#ifndef UGLAD_SIMT_EMUL
#include <dlfcn.h>
#endif
namespace {
struct RcclApi {
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, uglad_rccl_id, int) = nullptr;  // (ncclUniqueId travels by value: 128 bytes)
  int (*CommDestroy)(void*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;
  bool ok = false;
};
const RcclApi& rccl_api() {
  static const RcclApi api = [] {
    RcclApi a;
#ifndef UGLAD_SIMT_EMUL  // (the emulator build has no RCCL: never ok)
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so"})
      if (!h) h = dlopen(name, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);  // the copy PyTorch has loaded, if any
    for (const char* name : {"librccl.so.1", "librccl.so"})
      if (!h) h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (!h) return a;
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(h, "ncclAllReduce"));
    a.CommCount = reinterpret_cast<decltype(a.CommCount)>(dlsym(h, "ncclCommCount"));
    a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllReduce;
#endif
    return a;
  }();
  return api;
}
constexpr int kNcclFloat32 = 7, kNcclSum = 0;  // rccl.h: ncclDataType_t / ncclRedOp_t
}  // namespace
extern "C" {

int uglad_rccl_unique_id(uglad_rccl_id* id_out) {
  if (!id_out) return UGLAD_E_NULL;
  if (!rccl_api().ok) return UGLAD_E_RCCL;
  return rccl_api().GetUniqueId(id_out) == 0 ? 0 : UGLAD_E_RCCL;
}

int uglad_rccl_comm_init(const uglad_rccl_id* id, int nranks, int rank, void** comm_out) {
  if (!id || !comm_out) return UGLAD_E_NULL;
  if (nranks < 1 || rank < 0 || rank >= nranks) return UGLAD_E_DIM;
  if (!rccl_api().ok) return UGLAD_E_RCCL;
  return rccl_api().CommInitRank(comm_out, nranks, *id, rank) == 0 ? 0 : UGLAD_E_RCCL;
}

int uglad_rccl_comm_destroy(void* comm) {
  if (!comm) return UGLAD_E_NULL;
  if (!rccl_api().ok) return UGLAD_E_RCCL;
  return rccl_api().CommDestroy(comm) == 0 ? 0 : UGLAD_E_RCCL;
}

// ncclCommCount: how many ranks the communicator spans -- what a multi-GPU record can show to prove that RCCL saw all of them
int uglad_rccl_comm_count(void* comm, int* nranks_out) {
  if (!comm || !nranks_out) return UGLAD_E_NULL;
  if (!rccl_api().ok || !rccl_api().CommCount) return UGLAD_E_RCCL;
  return rccl_api().CommCount(comm, nranks_out) == 0 ? 0 : UGLAD_E_RCCL;
}

// (has the signature of uglad_allreduce_fn: hand its address and the communicator to uglad_glad_forward_sharded)
int uglad_rccl_allreduce_sum(float* buf, int n, void* comm, uglad_stream_t stream) {
  if (!buf || !comm) return UGLAD_E_NULL;
  if (n < 1) return UGLAD_E_DIM;
  if (!rccl_api().ok) return UGLAD_E_RCCL;
  return rccl_api().AllReduce(buf, buf, (size_t)n, kNcclFloat32, kNcclSum, comm, (hipStream_t)stream) == 0 ? 0 : UGLAD_E_RCCL;
}

}  // extern "C"
