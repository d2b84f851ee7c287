// mfm_comm.hpp -- the all-reduce of a row-sharded fit: the two providers (caller's callback, RCCL bound at run time) and
// the per-context communicator with its call and double counters. Shared by the Gibbs context (mfm_hip.hip through
// mfm_plan.hpp) and the variational context (mfm_vb.hip).
#pragma once
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include <dlfcn.h>

#include "mfm_common.hpp"

struct mfm_nccl_id {
  char internal[128];  // ncclUniqueId (NCCL_UNIQUE_ID_BYTES)
};

namespace mfm {

// In-place sum over the ranks of `count` doubles in device memory, enqueued in order on the ctx stream.
typedef int (*mfm_allreduce_fn)(void *user, void *dev_buf, int64_t count);
// Two providers: a caller-supplied callback (mfm_set_allreduce: e.g. torch.distributed on the ctx stream), or RCCL called
// from this library on the ctx stream (mfm_comm_init: ncclAllReduce over xGMI, no interpreter in the loop). librccl is
// bound at run time (dlopen) so that single-GPU use does not depend on it.
struct Rccl {
  void *lib = nullptr;
  std::string path;  // where the bound librccl lives (dladdr of ncclAllReduce)
  int (*GetUniqueId)(void *) = nullptr;
  int (*CommInitRank)(void **, int, mfm_nccl_id, int) = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*CommCount)(void *, int *) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  // Resolution order: (1) a librccl the process has already mapped (a torch process: torch/lib/librccl.so -- two RCCL copies
  // in one process would each open their own xGMI rings), (2) the directory the HIP runtime in use was loaded from (a wheel
  // that bundles libamdhip64 bundles its RCCL next to it), (3) the dynamic loader's search path, (4) /opt/rocm/lib.
  static void *open_any() {
    static const char *names[] = {"librccl.so.1", "librccl.so"};
    for (const char *n : names)
      if (void *h = dlopen(n, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD)) return h;
    Dl_info di;
    if (dladdr((const void *)&hipGetDeviceCount, &di) && di.dli_fname) {
      std::string dir(di.dli_fname);
      const size_t slash = dir.rfind('/');
      if (slash != std::string::npos) {
        dir.resize(slash + 1);
        for (const char *n : names)
          if (void *h = dlopen((dir + n).c_str(), RTLD_NOW | RTLD_GLOBAL)) return h;
      }
    }
    for (const char *n : names)
      if (void *h = dlopen(n, RTLD_NOW | RTLD_GLOBAL)) return h;
    for (const char *n : {"/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"})
      if (void *h = dlopen(n, RTLD_NOW | RTLD_GLOBAL)) return h;
    return nullptr;
  }
  static Rccl &get() {
    static Rccl r;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (!r.lib) {
      void *h = open_any();
      if (!h) throw Error(MFM_ERR_RUNTIME, std::string("cannot load librccl.so: ") + dlerror());
      r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
      r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
      r.AllReduce = (decltype(r.AllReduce))dlsym(h, "ncclAllReduce");
      r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
      r.CommCount = (decltype(r.CommCount))dlsym(h, "ncclCommCount");
      r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
      if (!r.GetUniqueId || !r.CommInitRank || !r.AllReduce || !r.CommDestroy)
        throw Error(MFM_ERR_RUNTIME, "librccl.so lacks the expected entry points");
      Dl_info di;
      if (dladdr((const void *)r.AllReduce, &di) && di.dli_fname) r.path = di.dli_fname;
      r.lib = h;
    }
    return r;
  }
  void check(int rc, const char *what) const {
    if (rc != 0)
      throw Error(MFM_ERR_RUNTIME, std::string(what) + " failed: " + (GetErrorString ? GetErrorString(rc) : "rccl error"));
  }
};

struct Comm {
  mfm_allreduce_fn fn = nullptr;
  void *user = nullptr;
  void *nccl = nullptr;        // ncclComm_t (mfm_comm_init)
  hipStream_t stream = nullptr;  // the ctx stream the native collective is enqueued on
  int rank = 0, world = 1;
  bool shard_set = false;  // mfm_set_shard / mfm_comm_init told us this rank's place (else: rank 0 <=> row offset 0)
  mutable int64_t calls = 0, doubles = 0;
  bool active() const { return fn != nullptr || nccl != nullptr; }
  void allreduce(void *buf, int64_t count) const {
    if (count <= 0 || !active()) return;
    calls++;
    doubles += count;
    if (nccl) {
      Rccl &r = Rccl::get();
      r.check(r.AllReduce(buf, buf, (size_t)count, /*ncclDouble*/ 8, /*ncclSum*/ 0, nccl, stream), "ncclAllReduce");
      return;
    }
    if (fn(user, buf, count) != 0) throw Error(MFM_ERR_RUNTIME, "all-reduce callback failed");
  }
  // The ranks' agreement at setup: v summed over the ranks, the result on the host (s: the ctx stream the collective runs on).
  // Every rank must come here with the same length at the same point, or all of them wait for ever.
  void sum_ranks(std::vector<double> &v, hipStream_t s) const {
    DevBuf<double> d;
    d.upload(v);
    allreduce(d.p, (int64_t)v.size());
    MFM_HIP_CHECK(hipStreamSynchronize(s));
    MFM_HIP_CHECK(hipMemcpy(v.data(), d.p, v.size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  // ... and a vote: did every rank say yes?
  bool all_ranks(bool yes, hipStream_t s) const {
    std::vector<double> no{yes ? 0.0 : 1.0};
    sum_ranks(no, s);
    return no[0] == 0.0;
  }
  ~Comm() {
    if (nccl) (void)Rccl::get().CommDestroy(nccl);
  }
};

}  // namespace mfm
