// What every handle and entry of the library's host layer (api.hip) shares: the error type and the HIPCHK / RBCHK checks, the
// reference-counted device buffer, the event pair of the timed entries, the NNSDP_* environment reads, the rocBLAS handle and the
// lazily loaded RCCL.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <dlfcn.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <future>
#include <memory>
#include <string>
#include <vector>

#include "../../include/nnsdp.h"

namespace nnsdp {

thread_local std::string g_err;

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess)                                                                           \
      throw HipError(std::string(#x) + " failed: " + hipGetErrorString(e_) + " (" __FILE__ ":" +    \
                     std::to_string(__LINE__) + ")");                                               \
  } while (0)
#define RBCHK(x)                                                                                    \
  do {                                                                                              \
    rocblas_status s_ = (x);                                                                        \
    if (s_ != rocblas_status_success)                                                               \
      throw HipError(std::string(#x) + " failed: rocblas_status " + std::to_string((int)s_));       \
  } while (0)

static double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

template <class T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  // the allocation is reference-counted: the members of a solver family (nnsdp_solver_create_sibling) hold the same set-up
  // buffers, and the last holder frees them
  std::shared_ptr<void> own;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  void release() { own.reset(); p = nullptr; }
  void adopt(void* q) { own = std::shared_ptr<void>(q, [](void* x) { (void)hipFree(x); }); p = static_cast<T*>(q); }
  void alloc(size_t count) {
    release();
    n = count;
    if (count) { void* q = nullptr; HIPCHK(hipMalloc(&q, count * sizeof(T))); adopt(q); }
  }
  // a second holder of o's allocation (read-only use)
  void share(const DBuf& o) { own = o.own; p = o.p; n = o.n; }
  size_t bytes() const { return p ? n * sizeof(T) : 0; }
  bool shared() const { return own && own.use_count() > 1; }
  // fine-grained device memory: coherent across devices WHILE kernels run (the hipIpc exchange buffers: a peer's kernel polls a flag
  // and reads data another device's kernel is publishing; coarse-grained memory only promises that at kernel boundaries)
  bool alloc_finegrained(size_t count) {
    release();
    n = count;
    void* q = nullptr;
    if (hipExtMallocWithFlags(&q, count * sizeof(T), hipDeviceMallocFinegrained) != hipSuccess) { (void)hipGetLastError(); n = 0; return false; }
    adopt(q);
    return true;
  }
  void upload(const std::vector<T>& h) {
    alloc(h.size());
    if (!h.empty()) HIPCHK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  void zero() { if (n) HIPCHK(hipMemset(p, 0, n * sizeof(T))); }
  std::vector<T> download() const {
    std::vector<T> h(n);
    if (n) HIPCHK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
};

static void require_gpu() {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt <= 0)
    throw HipError("no HIP device available: libnnsdp_hip has no CPU fallback (the product path is GPU-only)");
}

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// the two events around the timed launches of a one-shot entry: destroyed on every path out of it, HIPCHK throws
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  void create() { HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1)); }
  ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

// the NNSDP_* environment overrides (diagnostics and test hooks): set at all / set to a non-zero integer / a number or the default.
// A caller that wants one read per process keeps the result in a function-local static const.
static bool env_set(const char* name) { return std::getenv(name) != nullptr; }
static bool env_flag(const char* name) { const char* e = std::getenv(name); return e && std::atoi(e) != 0; }
static long long env_int(const char* name, long long dflt) { const char* e = std::getenv(name); return e ? std::atoll(e) : dflt; }
static double env_real(const char* name, double dflt) { const char* e = std::getenv(name); return e ? std::atof(e) : dflt; }

// RCCL is loaded lazily (dlopen) and only in clique-sharded mode, so the default single-GPU / replica paths
// never touch it.  Minimal declarations matching /opt/rocm/include/rccl/rccl.h.
struct Rccl {
  struct UniqueId { char internal[128]; };
  typedef void* Comm;
  int (*GetUniqueId)(UniqueId*) = nullptr;
  int (*CommInitRank)(Comm*, int, UniqueId, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, Comm, hipStream_t) = nullptr;
  int (*CommDestroy)(Comm) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  static constexpr int kFloat64 = 8, kSum = 0;
  static Rccl& get() {
    static Rccl r;
    if (!r.GetUniqueId) {
      void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
      if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
      if (!h) throw HipError(std::string("cannot load RCCL: ") + dlerror());
      auto sym = [&](const char* n) { void* p = dlsym(h, n); if (!p) throw HipError(std::string("RCCL symbol missing: ") + n); return p; };
      r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
      r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
      r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
      r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
      r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
    }
    return r;
  }
  void check(int rc, const char* what) {
    if (rc != 0) throw HipError(std::string(what) + " failed: " + (GetErrorString ? GetErrorString(rc) : "?"));
  }
};

struct RocHandle {
  rocblas_handle h = nullptr;
  RocHandle() {
    RBCHK(rocblas_create_handle(&h));
    // reproducible library results: no atomics-based (split-K) accumulation inside rocBLAS / rocSOLVER.  M^-1, the certificate
    // polish and the eigmax check are then the same bits run to run and rank to rank on one GPU model
    RBCHK(rocblas_set_atomics_mode(h, rocblas_atomics_not_allowed));
  }
  ~RocHandle() { if (h) rocblas_destroy_handle(h); }
};

}  // namespace nnsdp
