// C ABI of libohxgb.so (include/ohxgb.h): the XGBoost C-API symbols that
// QuickChem's Shared/xgb_fortran_api.F90 binds, served by the gfx950 kernels,
// plus the device-resident and fused entry points.
//
// Host logic only: handle bookkeeping, model load/save, lazy upload of the
// flattened booster to HBM, staging and launches.  No prediction arithmetic
// happens on the CPU anywhere in this library.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <atomic>
#include <chrono>
#include <mutex>
#include <unordered_map>
#include <sstream>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/ohxgb.h"
#include "categorical.hpp"
#include "cells.hpp"
#include "contribs.hpp"
#include "flatten.hpp"
#include "forest.hpp"
#include "groups.hpp"
#include "kernels.hpp"
#include "visits.hpp"
#include "refit.hpp"
#include "grow.hpp"
#include "grow_quantile.hpp"
#include "cuts.hpp"

using namespace ohx;

namespace {

thread_local std::string g_last_error;

void set_error(const std::string& m) { g_last_error = m; }

}  // namespace

namespace ohx {
void set_last_error(const std::string& m) { g_last_error = m; }   // for comm.cpp
}

namespace {

#define API_BEGIN() try {
#define API_END()                                   \
  }                                                 \
  catch (const std::exception& e) {                 \
    set_error(e.what());                            \
    return -1;                                      \
  }                                                 \
  catch (...) {                                     \
    set_error("unknown error");                     \
    return -1;                                      \
  }                                                 \
  return 0;

#define HIP_CHECK(expr)                                                                            \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) throw OhxError(std::string(#expr) + " failed: " + hipGetErrorString(e_)); \
  } while (0)

// Handles are checked against the set of live objects, never by reading the object: the reference frees its
// DMatrix every step (OH_GridCompMod.F90:377), so a stale handle points at memory the allocator has long
// handed to someone else.
struct HandleRegistry {
  std::mutex mu;
  std::unordered_set<const void*> live;
  void add(const void* p) {
    std::lock_guard<std::mutex> g(mu);
    live.insert(p);
  }
  bool has(const void* p) {
    std::lock_guard<std::mutex> g(mu);
    return live.count(p) != 0;
  }
  bool remove(const void* p) {
    std::lock_guard<std::mutex> g(mu);
    return live.erase(p) != 0;
  }
};
HandleRegistry g_dmats, g_boosters;

// ------------------------------------------------------------------ device

struct DeviceInfo {
  int ordinal = -1;
  int num_cus = 0;
};

int device_count_or_throw() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    throw OhxError(std::string("libohxgb needs a HIP device and has no CPU fallback: hipGetDeviceCount: ") +
                   (e != hipSuccess ? hipGetErrorString(e) : "0 devices"));
  return n;
}

DeviceInfo use_device(int ordinal) {
  const int n = device_count_or_throw();
  if (ordinal < 0) {
    int cur = 0;
    HIP_CHECK(hipGetDevice(&cur));
    ordinal = cur;
  }
  if (ordinal >= n) throw OhxError("HIP device ordinal " + std::to_string(ordinal) + " out of range");
  HIP_CHECK(hipSetDevice(ordinal));
  DeviceInfo d;
  d.ordinal = ordinal;
  int cus = 0;
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ordinal));
  d.num_cus = cus > 0 ? cus : 256;
  return d;
}

// The two streams everything of this library runs on (per device, made at first use, kept for the life of the process):
// `exec` for kernels and whatever must stay in order with them, `copy` for PCIe transfers that run beside them.  None of
// the library's own work goes to the null stream, and no object has streams of its own: every stream a process has ever
// used is a hardware queue the GPU's scheduler keeps mapped, and a GPU shared by several MPI ranks - how GEOS runs -
// time-slices queues once there are more of them than it has slots.  Six ranks with four queues each: a tick in a
// hundred took 14-37 ms instead of 1; with two each, none did (profiles/r05_sweeps.txt, "six ranks").
struct LibStreams {
  hipStream_t exec = nullptr, copy = nullptr;
  hipEvent_t caller = nullptr;      // order_behind_caller
};
LibStreams& lib_streams(int ordinal) {
  static std::mutex mu;
  static std::unordered_map<int, LibStreams> by_device;
  std::lock_guard<std::mutex> g(mu);
  LibStreams& ls = by_device[ordinal];
  if (ls.exec == nullptr) {
    int cur = 0;
    HIP_CHECK(hipGetDevice(&cur));
    if (cur != ordinal) HIP_CHECK(hipSetDevice(ordinal));
    HIP_CHECK(hipStreamCreateWithFlags(&ls.exec, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&ls.copy, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&ls.caller, hipEventDisableTiming));      // made here, under the lock: two threads may ask
    if (cur != ordinal) HIP_CHECK(hipSetDevice(cur));
  }
  return ls;
}
// A host-form call on a matrix that BORROWS the caller's HBM (OHXDMatrixCreateFromDevice): whatever the caller has
// enqueued on the legacy default stream - and so on every blocking stream, torch's default among them - to fill those
// rows must be there before the library's non-blocking stream reads them.  The null-stream launch these calls made
// until round 4 gave that order by itself.  An event on the default stream, waited for by `s`; nothing of
// the library runs on the default stream.  A producer on a NON-blocking stream of the caller's is the caller's to
// synchronise (include/ohxgb.h), or to name: the *Device forms take the stream.
void order_behind_caller(int ordinal, hipStream_t s) {
  // (one event per device, re-recorded by every such call: a wait takes the event's state as it is when the wait is
  // enqueued, so a later record does not disturb an earlier call's wait; two threads at once serialise here - the pair
  // record + wait must not interleave with another thread's)
  static std::mutex mu;
  LibStreams& ls = lib_streams(ordinal);
  std::lock_guard<std::mutex> g(mu);
  HIP_CHECK(hipEventRecord(ls.caller, nullptr));
  HIP_CHECK(hipStreamWaitEvent(s, ls.caller, 0));
}
// the current device's
hipStream_t exec_stream() {
  int cur = 0;
  HIP_CHECK(hipGetDevice(&cur));
  return lib_streams(cur).exec;
}

// Owns its allocation: movable (a std::vector of them may reallocate), never copied - a copy would free the same
// pointer twice and leave the survivor pointing at freed memory.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) {
    o.p = nullptr;
    o.n = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      n = o.n;
      o.p = nullptr;
      o.n = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void ensure(size_t count) {
    if (count <= n) return;
    release();
    try {
      HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T)));
    } catch (const OhxError&) {
      (void)hipGetLastError();   // forgotten here: left with the runtime, it would surface again as the error of the next launch
      throw;
    }
    n = count;
  }
  void upload(const std::vector<T>& h) {
    ensure(h.size());
    if (h.empty()) return;
    hipStream_t s = exec_stream();
    HIP_CHECK(hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));      // `h` is the caller's again
  }
};

template <class T>
struct PinnedBuf {
  T* p = nullptr;
  size_t n = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;             // owns its allocation, as DevBuf
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  void ensure(size_t count) {
    if (count <= n) return;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
    try {
      HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault));
    } catch (const OhxError&) {
      (void)hipGetLastError();   // as DevBuf::ensure
      throw;
    }
    n = count;
  }
};

// ------------------------------------------------------------------ objects

// Freed matrix buffers are parked here and handed to the next XGDMatrixCreateFromMat that fits: the
// reference creates and frees its DMatrix on every OH tick (OH_GridCompMod.F90:347,377), and a hipMalloc +
// hipFree of the whole batch per tick costs more than the prediction of a small sub-domain.  At most
// kSlots buffers are kept; OHXReleaseScratch() (or OHX_DMATRIX_POOL=0 in the environment) returns them.
struct RowPool {
  static constexpr size_t kSlots = 2;
  struct Slot {
    float* p;
    size_t n;
    int device;
  };
  std::mutex mu;
  std::vector<Slot> slots;
  bool enabled() const {
    static const bool on = [] {
      const char* e = getenv("OHX_DMATRIX_POOL");
      return !(e && e[0] == '0');
    }();
    return on;
  }
  // a buffer of at least `count` floats on `device`; *cap = what it really holds
  float* take(size_t count, int device, size_t* cap) {
    {
      std::lock_guard<std::mutex> g(mu);
      size_t best = slots.size();
      for (size_t i = 0; i < slots.size(); ++i)
        if (slots[i].device == device && slots[i].n >= count && slots[i].n <= 4 * count + (1u << 18) &&
            (best == slots.size() || slots[i].n < slots[best].n))
          best = i;
      if (best != slots.size()) {
        Slot sl = slots[best];
        slots.erase(slots.begin() + (long)best);
        *cap = sl.n;
        return sl.p;
      }
    }
    float* p = nullptr;
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(float)));
    *cap = std::max<size_t>(count, 1);
    return p;
  }
  void give(float* p, size_t cap, int device) {
    if (p == nullptr) return;
    if (enabled()) {
      std::lock_guard<std::mutex> g(mu);
      slots.push_back({p, cap, device});
      if (slots.size() <= kSlots) return;
      size_t drop = 0;                                  // keep the biggest
      for (size_t i = 1; i < slots.size(); ++i)
        if (slots[i].n < slots[drop].n) drop = i;
      p = slots[drop].p;
      device = slots[drop].device;
      slots.erase(slots.begin() + (long)drop);
    }
    (void)hipFree(p);
  }
  void release_all() {
    std::lock_guard<std::mutex> g(mu);
    for (Slot& sl : slots) (void)hipFree(sl.p);
    slots.clear();
  }
};
RowPool g_row_pool;

// The caller's host arrays, registered with the driver (ohx_register_host = 1; include/ohxgb.h part 2).
//
// The host forms of the fused calls copy some forty arrays per OH tick (OHXBoosterRun1: 37 inputs, up to 12 outputs).
// From pageable memory every one of those copies is a staged, synchronous transfer: on a GEOS-sized rank block
// (48 x 24 x 72) they cost more than the prediction (profiles/r04_ranks_per_gpu*.json).  A registered (pinned) array
// is read and written by the GPU's DMA engines directly and `hipMemcpyAsync` returns at once.  Registration costs
// about as much as ten ticks and is done once per array: (pointer, bytes) is remembered, and MAPL's import, export
// and internal pointers are the same from tick to tick (OH_GridCompMod.F90:1136,1195: MAPL_GetPointer on states that
// live as long as the run).  It is OPT-IN because it is a contract: an array that was passed while this is on must
// stay allocated until OHXUnregisterHost(array), OHXReleaseScratch() or the end of the process.  What happens to an
// array that is freed while registered is the driver's business, not this table's: ROCm pins registered ranges
// through KFD userptr objects that follow the process's page tables (a range that is unmapped is invalidated, a later
// GPU access to it faults; one that is mapped again is pinned again), so the failure is loud rather than stale - but
// it is a failure, hence the contract, and hence OHXUnregisterHost for a caller whose arrays do come and go.
// Nothing is unregistered while a copy may be in flight: the device is synchronised first.  What the driver
// refuses to register (it happens to ranges that share a page with another registration) is copied the pageable way
// as before.
struct HostRegistry {
  std::mutex mu;
  std::atomic<bool> on{false};
  struct Pin {
    size_t bytes;
    void* mapped;      // where the GPU sees the array (hipHostGetDevicePointer, asked once)
  };
  std::unordered_map<const void*, Pin> pinned;        // base -> what we registered
  std::unordered_map<const void*, size_t> refused;    // base -> bytes the driver would not take
  size_t bytes = 0;
  // true when [p, p + n) is registered afterwards; *mapped (optional) = the address the GPU reaches it at, or null
  bool want(const void* p, size_t n, void** mapped = nullptr) {
    if (mapped) *mapped = nullptr;
    if (!on.load(std::memory_order_relaxed) || p == nullptr || n == 0) return false;
    std::lock_guard<std::mutex> g(mu);
    auto it = pinned.find(p);
    if (it != pinned.end()) {
      if (it->second.bytes >= n) {
        if (mapped) *mapped = it->second.mapped;
        return true;
      }
      (void)hipDeviceSynchronize();                       // no copy of the old range may still be in flight
      (void)hipHostUnregister(const_cast<void*>(p));      // the same array, grown: again from the start
      bytes -= it->second.bytes;
      pinned.erase(it);
    }
    auto rf = refused.find(p);
    if (rf != refused.end() && rf->second == n) return false;
    if (hipHostRegister(const_cast<void*>(p), n, hipHostRegisterDefault) != hipSuccess) {
      (void)hipGetLastError();
      refused[p] = n;
      return false;
    }
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, const_cast<void*>(p), 0) != hipSuccess) {
      (void)hipGetLastError();
      dev = nullptr;
    }
    pinned[p] = Pin{n, dev};
    bytes += n;
    if (mapped) *mapped = dev;
    return true;
  }
  void release_all() {
    std::lock_guard<std::mutex> g(mu);
    if (getenv("OHX_REGISTRY_LOG") && (!pinned.empty() || !refused.empty()))
      fprintf(stderr, "[ohxgb] host registry: %zu arrays (%zu bytes) registered, %zu refused\n", pinned.size(), bytes,
              refused.size());
    if (!pinned.empty()) (void)hipDeviceSynchronize();     // DMA targets are not unpinned under a running copy
    for (auto& kv : pinned) (void)hipHostUnregister(const_cast<void*>(kv.first));
    pinned.clear();
    refused.clear();
    bytes = 0;
  }
  // one array leaves (OHXUnregisterHost): true if it was registered
  bool forget(const void* p) {
    std::lock_guard<std::mutex> g(mu);
    refused.erase(p);
    auto it = pinned.find(p);
    if (it == pinned.end()) return false;
    (void)hipDeviceSynchronize();
    (void)hipHostUnregister(const_cast<void*>(p));
    bytes -= it->second.bytes;
    pinned.erase(it);
    return true;
  }
};
HostRegistry g_host_registry;

// Host arrays <-> HBM for the host forms of the fused calls.  Arrays the registry holds are gathered into ONE launch of
// copy_arrays_kernel (the GPU reads or writes the caller's memory over PCIe itself) as long as the whole list is
// small - a rank-sized block, where forty separate copies cost forty fixed prices; big lists and arrays that are not
// registered go through hipMemcpyAsync.
// blocks of a launch of copy_arrays_kernel, over all its arrays ("ohx_copy_blocks"; 0 = as many as an array has 1 KiB
// pieces, up to 2 048 per array).  Sixty-four: a copy kernel that fills the chip with waves waiting on PCIe is slower at
// moving a rank's arrays (88 against 72 us per 3.7 MB list) and - with megabytes of reads queued on the link - keeps
// every other queue's kernels from STARTING until it is done (the command processor fetches their packets and
// arguments over the same link); a 48 x 24 x 72 tick 0.349 / 0.345 / 0.328 / 0.339 / 0.389 ms at 256 / 128 / 64 / 32 / 16
// blocks, 0.398 with a block per KiB (profiles/r05_sweeps.txt)
std::atomic<uint32_t> g_copy_blocks{64};
// "ohx_copy_engine" (process-wide): how REGISTERED host arrays cross.  kernel (default) = lists by copy_arrays_kernel (one
// launch per list; the one list that crosses under the walk by DMA, OHX_COPY_POST_BLOCKS); dma = every array by
// hipMemcpyAsync (the DMA engines: a fixed price per array, no wave on any CU); auto = OHXBoosterRun1's host form times
// its own ticks both ways and keeps the faster (CopyEngineTrial below), everything else as kernel.
// Round 5 supposed that DMA would win once ranks share the card (a copy kernel's waves, waiting on PCIe on every CU, hold
// up the other ranks' walks).  Measured (profiles/r06_ranks_per_gpu_block_48x24_engines.json, a 48 x 24 x 72 tick at 1 / 2 / 3 / 6
// ranks): copy kernels 0.290 / 0.583 / 0.678 / 1.348 ms, all by DMA 0.614 / 1.258 / 1.738 / 3.131 ms - forty fixed prices
// a tick lose at every count, auto picked "kernel" on every rank of every run, and its trial's eight DMA ticks are what
// its p99 is made of (3.8 against 1.9 ms at six ranks).  So kernel is the default and auto is there to be asked for.
enum CopyEngine : int { kCopyKernel = 0, kCopyDma = 1, kCopyAuto = 2 };
std::atomic<int> g_copy_engine{kCopyKernel};
struct HostMover {
  static constexpr size_t kKernelBytesMax = 64u << 20;
  CopyList list;
  size_t list_bytes = 0;
  hipStream_t stream;
  bool to_device;
  uint32_t blocks_override = 0;       // blocks of this mover's launches, when its owner knows better than the defaults
  bool by_dma;                        // registered arrays too go through hipMemcpyAsync (the DMA engines: no wave on a CU)
  explicit HostMover(hipStream_t s, bool h2d)
      : stream(s), to_device(h2d), by_dma(g_copy_engine.load(std::memory_order_relaxed) == kCopyDma) {}
  void add(float* dst, const float* src, size_t count) {
    if (count == 0) return;
    const void* host = to_device ? (const void*)src : (const void*)dst;
    void* mapped = nullptr;
    if (g_host_registry.want(host, count * sizeof(float), &mapped) && mapped != nullptr && !by_dma && list.count < kCopyListMax &&
        list_bytes + count * sizeof(float) <= kKernelBytesMax) {
      list.src[list.count] = to_device ? static_cast<const float*>(mapped) : src;
      list.dst[list.count] = to_device ? dst : static_cast<float*>(mapped);
      list.n[list.count] = count;
      ++list.count;
      list_bytes += count * sizeof(float);
      return;
    }
    (void)hipGetLastError();
    HIP_CHECK(hipMemcpyAsync(dst, src, count * sizeof(float), to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, stream));
  }
  // `count` floats at `offset` of a host array of `whole` floats that is registered as a whole (a k-slab of a MAPL field)
  void add_slice(float* dev, const float* host_base, size_t whole, size_t offset, size_t count) {
    if (count == 0) return;
    void* mapped = nullptr;
    if (g_host_registry.want(host_base, whole * sizeof(float), &mapped) && mapped != nullptr && !by_dma && list.count < kCopyListMax &&
        list_bytes + count * sizeof(float) <= kKernelBytesMax) {
      float* m = static_cast<float*>(mapped) + offset;
      list.src[list.count] = to_device ? m : dev;
      list.dst[list.count] = to_device ? dev : m;
      list.n[list.count] = count;
      ++list.count;
      list_bytes += count * sizeof(float);
      return;
    }
    (void)hipGetLastError();
    float* host = const_cast<float*>(host_base) + offset;
    HIP_CHECK(hipMemcpyAsync(to_device ? (void*)dev : (void*)host, to_device ? (const void*)host : (const void*)dev,
                             count * sizeof(float), to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, stream));
  }
  // a few words between HBM and pinned memory of the library's own (hipHostMalloc: the GPU reaches it at its host address),
  // riding on the list's launch; false when the list is full or empty - the caller copies them its own way then
  bool ride(void* dst, const void* src, size_t words) {
    if (list.count == 0 || list.count >= kCopyListMax) return false;
    list.src[list.count] = static_cast<const float*>(src);
    list.dst[list.count] = static_cast<float*>(dst);
    list.n[list.count] = words;
    ++list.count;
    return true;
  }
  void go() {
    // a launch that WRITES the caller's memory runs at a tick's end with nothing beside it to keep from starting, and posted
    // writes want more waves than reads do: 512 blocks (OHX_COPY_BACK_BLOCKS, read once; 0 = as many as ohx_copy_blocks).
    // A rank's tick at 64 / 128 / 256 / 512: 0.309 / 0.309 / 0.306 / 0.303 ms (profiles/r05_sweeps.txt)
    static const int back_blocks = [] { const char* e = getenv("OHX_COPY_BACK_BLOCKS"); return e ? atoi(e) : 512; }();
    uint32_t blocks = (!to_device && back_blocks > 0) ? (uint32_t)back_blocks : g_copy_blocks.load(std::memory_order_relaxed);
    if (blocks_override > 0) blocks = blocks_override;
    if (list.count == 0) return;
    HIP_CHECK(launch_copy_arrays(list, stream, blocks));
    list.count = 0;
    list_bytes = 0;
  }
};

// host -> device, through the registry when it is on (then asynchronous on `stream`), the pageable way otherwise
void upload_host_array(float* dst, const float* src, size_t count, hipStream_t stream) {
  if (count == 0) return;
  (void)g_host_registry.want(src, count * sizeof(float));
  HIP_CHECK(hipMemcpyAsync(dst, src, count * sizeof(float), hipMemcpyHostToDevice, stream));
}
// device -> host; the caller synchronises `stream` before it looks at dst
void download_host_array(float* dst, const float* src, size_t count, hipStream_t stream) {
  if (count == 0) return;
  (void)g_host_registry.want(dst, count * sizeof(float));
  HIP_CHECK(hipMemcpyAsync(dst, src, count * sizeof(float), hipMemcpyDeviceToHost, stream));
}

// Flag and verdict words of the matrix checks (inf scan, level-size search): one device buffer and one pinned
// host mirror per process, so that a check is launches + ONE read-back.
struct CheckScratch {
  std::mutex mu;
  int device = -1;
  DevBuf<uint32_t> d;
  PinnedBuf<uint32_t> h;
  void ensure(size_t words, int dev) {
    if (dev != device) {
      d.release();
      device = dev;
    }
    d.ensure(words);
    h.ensure(words);
  }
};
CheckScratch g_check;

struct DMatrixObj {
  ~DMatrixObj() {
    // XGBoosterPredict has waited for its kernels; OHXBoosterPredictDevice only enqueues on the caller's stream, and the
    // next XGDMatrixCreateFromMat copies into a parked buffer on the library's: not before the readers are done
    if (owned != nullptr && used_async) {
      (void)hipSetDevice(device);
      (void)hipDeviceSynchronize();
    }
    g_row_pool.give(owned, owned_cap, device);
  }
  bool used_async = false;
  uint64_t nrow = 0, ncol = 0;
  float missing = NAN;
  const float* d_data = nullptr;  // device
  float* owned = nullptr;         // set when the matrix owns its storage (XGDMatrixCreateFromMat)
  size_t owned_cap = 0;
  int device = -1;
  // OHXDMatrixSetGrid: the rows are grid rows grid_row0 .. of an (im,jm,*) grid; 0 = not said
  int grid_im = 0, grid_jm = 0;
  uint64_t grid_row0 = 0;
  bool grid_inferred = false;     // found by infer_level_size, not said by the caller
  bool grid_looked = false;       // the rows have been searched (or the caller has spoken): do not look again
  // rows in no known order: has the clustering pass been judged worth it for this matrix, and was it?
  bool cluster_decided = false, cluster_on = false;
};

// Per-feature contributions (OHXBoosterPredictContribs): tables built at the first contribs call of each mode on the
// loaded model, and buffers of their own - never one the predict, fields or Run1 paths use (a captured graph holds raw
// pointers to those).  Dropped with the model (adopt_model) and with the booster, and the device part of it when the
// booster has moved to another device ("ohx_device"); OHXReleaseScratch leaves them alone.
struct ContribsState {
  bool checked = false;              // feature count and cover checked, node means computed
  std::string error;                 // why this model cannot have contributions at all (no cover, too many features)
  std::string exact_error;           // why it cannot have exact ones (a path over too many distinct features)
  std::vector<std::vector<float>> means;
  int device = -1;                   // where the device part below lives
  bool exact_ready = false, approx_ready = false;
  DevBuf<PathHead> d_heads;          // exact mode: the path table
  DevBuf<PathElem> d_elems;
  DevBuf<uint32_t> d_class_start;
  DevBuf<float> d_coef;
  DevBuf<ContribNode> d_nodes;       // approximate mode
  DevBuf<uint32_t> d_roots;
  // the host form's output; the per-tree partials of split launches (sized by the largest split so far, at most
  // 1 GiB - contribs.hip kPartBudgetBytes); the host form's inf flag
  DevBuf<float> d_out, d_part;
  DevBuf<uint32_t> d_flags;
  PinnedBuf<float> h_out;
  PinnedBuf<uint32_t> h_flags;
  // SHAP interaction values (OHXBoosterPredictInteractions) share the tables above and have buffers of their own: the
  // feature-path index (exact mode, built at the first exact interactions call), the contributions phi, the partials
  // of both split launches, the host form's output and its host copy
  bool index_ready = false;
  DevBuf<uint32_t> d_fpaths, d_fstart;
  DevBuf<float> d_iphi, d_ipart, d_iout;
  PinnedBuf<float> h_iout;
  // the fields form's host form (OHXBoosterPredictContribsFields): the staged slab, one buffer per field, and the
  // requested outputs, one slab of gridcells each (its split launches use d_part above)
  std::vector<DevBuf<float>> d_fstage;
  DevBuf<float> d_fout;
  // several output groups: one group's block, [nrow][F+1] or [nrow][F+1][F+1], before it is scattered into the output
  DevBuf<float> d_gblock;
  void release_device() {
    for (DevBuf<float>* f : {&d_coef, &d_out, &d_part, &d_iphi, &d_ipart, &d_iout, &d_fout, &d_gblock}) f->release();
    d_fstage.clear();
    d_fpaths.release();
    d_fstart.release();
    index_ready = false;
    d_heads.release();
    d_elems.release();
    d_class_start.release();
    d_nodes.release();
    d_roots.release();
    d_flags.release();
    exact_ready = approx_ready = false;
    device = -1;
  }
};

// The forest as the walk to dense leaf indices reads it (visits.hpp VisitForest, DeviceLeafWalk): ONE per booster, read by
// the visit counts and by the leaf refit.  The host part is built by the first call of either on the loaded model and
// needs no device; the device part by the first count or refit.  Never a buffer of the predict, fields, Run1 or
// contributions paths, and read-only to every kernel: a device-form count still in flight and a later refit on the same
// device may read it together.  It holds no leaf value, so it outlives a refit; dropped - with the two states below -
// with the model (adopt_model), with the booster and by an "ohx_device" move; OHXReleaseScratch leaves all three alone.
// A booster without a device of its own follows the caller's current device: the walk is then freed and built again
// where it is asked for (hipFree waits for what still reads it), and each state below does the same with its own
// buffers when it next finds the walk elsewhere (`device`) - until then a count made on the old device stays readable.
struct LeafWalkState {
  VisitForest vf;                     // nodes, roots, leaf maps (host)
  int device = -1;                    // where the device part lives; -1 = not built yet
  int num_cus = 0;
  DevBuf<VisitNode> d_nodes;
  DevBuf<uint32_t> d_roots, d_leaf_offset;
};

// Node visit counts (OHXBoosterCountVisits): the plan's tree lists, the leaf counters and the buffers the results come
// back in.
struct VisitState {
  VisitPlan plan;                     // which trees take the LDS path, for the knobs below
  uint32_t plan_lds_leaves = 0;
  bool plan_use_lds = false, plan_uploaded = false;
  int device = -1;                    // the walk's device when the counters were made; -1 = not built yet
  DevBuf<uint32_t> d_lds_trees, d_global_trees;
  DevBuf<unsigned long long> d_counts;
  PinnedBuf<unsigned long long> h_leaf;
  std::vector<uint64_t> node_counts;  // what OHXBoosterGetVisitCounts hands out
  uint64_t rows_seen = 0;
};

// Leaf refit (OHXBoosterRefitLeaves; refit.hpp): the leaf-id planes, the running prediction, the per-leaf sums, the leaf
// tables and the staged labels.  Built at the first refit on the loaded model.
struct RefitState {
  int device = -1;                    // as VisitState's
  bool prepared = false;
  DevBuf<uint32_t> d_ids, d_error;
  DevBuf<float> d_pred, d_leaf, d_weight, d_labels;
  DevBuf<unsigned long long> d_G, d_H;
  PinnedBuf<float> h_leaf, h_weight;      // the old tables on the way in, the new ones on the way back
  PinnedBuf<unsigned long long> h_H;
  PinnedBuf<uint32_t> h_error;
};

// Boosting new trees (OHXBoosterBoostTrees; grow.hpp): the bin planes, the node a row stands on, the running margin, the
// level's histograms and candidates, the node records of every round and the staged labels and cuts.  Built at the
// first call on the loaded model; never a buffer of another path.
struct GrowState {
  int device = -1;
  bool prepared = false;               // prepare_grow has raised the LDS limits on `device`
  bool pairs_prepared = false;         // grow_lds_limits_pairs has: at the first call that takes the pair path
  bool quantile_prepared = false;      // grow_lds_limits_quantile has: at the first call under the quantile objective
  DevBuf<uint8_t> d_bins;
  DevBuf<uint16_t> d_pos;
  DevBuf<float> d_pred, d_labels, d_cuts;
  DevBuf<uint32_t> d_cut_ptr, d_tree_nodes, d_saved_flag;
  DevBuf<unsigned long long> d_Ghist, d_Hhist;
  DevBuf<GrowCand> d_best;
  DevBuf<GrowNode> d_nodes;
  DevBuf<GrowLevelState> d_state;
  PinnedBuf<GrowNode> h_nodes;
  PinnedBuf<uint32_t> h_tree_nodes, h_cut_ptr;
  PinnedBuf<float> h_cuts;
  PinnedBuf<GrowLevelState> h_state;
  // the held-out metric (OHXBoosterBoostTreesEval): the held-out rows' bin planes, margin and staged labels, and the
  // sums in the layout of the call's kind: [rounds + 1][2 sets][hi, lo], or with row weights W of both sets followed
  // by [rounds + 1][2 sets][p2, p1, p0]
  DevBuf<uint8_t> d_eval_bins;
  DevBuf<float> d_eval_pred, d_eval_labels;
  DevBuf<unsigned long long> d_sums;
  PinnedBuf<unsigned long long> h_sums;
  // row weights (OHXBoosterBoostTreesWeighted): the staged weights of both sets
  DevBuf<float> d_weights, d_eval_weights;
  // subsampling (OHXBoosterBoostTreesSampled): the bag's bit plane of the tree at hand, a bit a row, and the selected
  // features of every round [rounds][n_sel]
  DevBuf<unsigned long long> d_bag;
  DevBuf<uint8_t> d_features;
  PinnedBuf<uint8_t> h_features;
  // deep trees (OHXBoosterBoostTreesDeep with max_depth > 8): the uint32 positions of the levels from 8 on, and the tree
  // at hand as the held-out walk reads it
  DevBuf<uint32_t> d_pos_deep;
  DevBuf<uint8_t> d_eval_nodes;          // [node stride] x kGrowEvalNodeBytes
  // the pair path (grow_pairs.hip): the planes of the round at hand, 12 bytes a row, and the list 0 .. F - 1; allocated
  // only where the pair path runs
  DevBuf<long long> d_pair_q;
  DevBuf<uint32_t> d_pair_hq;
  DevBuf<uint8_t> d_identity;
  PinnedBuf<uint8_t> h_identity;
  // monotone constraints (grow_mono.hip): the weight intervals of the tree at hand, two doubles a node of the call's node
  // stride, and the constraints of every feature; allocated only where a constraint is active
  DevBuf<double> d_mono_bounds;
  DevBuf<int8_t> d_mono_constraints;
  PinnedBuf<int8_t> h_mono_constraints;
  // column sampling by level and by node (grow_colsample.hip): the lists of every round and level, [rounds][max_depth][n_lvl];
  // allocated only where a fraction takes a feature away
  DevBuf<uint8_t> d_level_lists;
  PinnedBuf<uint8_t> h_level_lists;
  // interaction constraints (grow_interact.hip): the sets of the tree at hand, four words a node of the call's node stride
  // (the features on its path, then those it may split on), and the groups, two words each; allocated only where the
  // constraints are active
  DevBuf<uint64_t> d_interact_sets;
  DevBuf<uint64_t> d_interact_groups;
  PinnedBuf<uint64_t> h_interact_groups;
  // the quantile objective (grow_quantile.hip): the bins of the select's pass at hand, 256 leaves x 256 digits x 8 bytes,
  // and its leaf table; allocated only where the objective runs
  DevBuf<uint8_t> d_quantile;
  void release_device() {
    d_quantile.release();
    d_level_lists.release();
    d_interact_sets.release();
    d_interact_groups.release();
    d_mono_bounds.release();
    d_mono_constraints.release();
    d_pair_q.release();
    d_pair_hq.release();
    d_identity.release();
    d_bag.release();
    d_features.release();
    d_pos_deep.release();
    d_eval_nodes.release();
    d_bins.release();
    d_pos.release();
    d_eval_bins.release();
    d_sums.release();
    for (DevBuf<float>* f : {&d_pred, &d_labels, &d_cuts, &d_eval_pred, &d_eval_labels, &d_weights, &d_eval_weights}) f->release();
    for (DevBuf<uint32_t>* f : {&d_cut_ptr, &d_tree_nodes, &d_saved_flag}) f->release();
    d_Ghist.release();
    d_Hhist.release();
    d_best.release();
    d_nodes.release();
    d_state.release();
    prepared = false;
    pairs_prepared = false;
    quantile_prepared = false;
  }
};

struct BoosterObj {
  ~BoosterObj() {
    for (hipEvent_t e : {run1_fork, run1_slab, run1_join, run1_clear})
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : run1_prep) (void)hipEventDestroy(e);
    for (hipEvent_t e : run1_walk) (void)hipEventDestroy(e);
    for (hipEvent_t e : run1_feed_events) (void)hipEventDestroy(e);
    if (train.side) (void)hipStreamDestroy(train.side);
    if (train.fork) (void)hipEventDestroy(train.fork);
    if (train.join) (void)hipEventDestroy(train.join);
    if (cluster_done) (void)hipEventDestroy(cluster_done);
    if (defer_seen) (void)hipEventDestroy(defer_seen);
  }
  TrainStreams train;              // second stream of the launch train (kernels.hpp): made when ohx_overlap_group asks for it
  Forest forest;                   // file order: what XGBoosterSaveModel writes
  // Several output groups (Forest::num_groups() >= 2, multi-class / multi-target): every device form is built from
  // `grouped`, the same trees ordered group by group (flatten.hpp group_major), so that group g is the tree range
  // [group_begin[g], group_begin[g+1]) of every walk and every contributions table.  A single-group booster has no copy:
  // flat() is `forest` itself, and its device forms are what they always were.
  uint32_t num_groups = 1;
  Forest grouped;
  std::vector<uint32_t> group_begin;     // G + 1 entries
  std::vector<uint32_t> flat_file_index; // file position of each tree of `grouped`
  const Forest& flat() const { return num_groups >= 2 ? grouped : forest; }
  bool loaded = false;
  float margin_base = 0.0f;        // Forest::margin_base() of the loaded model
  std::string margin_error;        // why it is unknown (objective this library cannot start a margin for)
  LayoutParams layout;
  std::string kernel_name = "auto";
  int device_pref = -1;
  LaunchTuning tune;
  // device state, built lazily at the first compute call
  bool uploaded = false;
  DeviceInfo dev;
  Placement placement;
  bool packed_ok = false;
  DevBuf<PackedNode> d_packed;
  DevBuf<WideNode> d_wide;
  DevBuf<SuperNode> d_super;
  DevBuf<SuperTreeHead> d_super_heads;
  bool super_ok = false;
  uint64_t super_slots = 0;
  uint64_t super_gathers[3] = {0, 0, 0};   // vector-memory instructions a wave issues to walk the whole forest once
                                        // without / with tree tops
  double super_mean_steps = 0.0;
  std::string symbol;                   // OHXBoosterKernelSymbol's answer
  DevBuf<uint32_t> d_roots;
  DevBuf<uint32_t> d_flags;
  uint32_t ring_reruns_seen = 0;        // of d_flags[1], as last read back; the first sighting is said on stderr
  DevBuf<float> d_leaves;               // small batches (kernels.hpp PredictArgs::leaf_buf): [tile][tree][lane] leaf values
  DevBuf<uint32_t> d_defer;             // deferred rows (kernels.hpp PredictArgs::defer_list): the count, then the list
  // how many rows of the last batch held missing values (read back behind the batch, looked at before the next one)
  PinnedBuf<uint32_t> h_defer_count;
  PinnedBuf<uint32_t> h_flags;          // d_flags[0..1] as the last copy-back kernel of a host-form tick left them
  hipEvent_t defer_seen = nullptr;
  bool defer_pending = false;
  uint64_t defer_last_nrow = 0;
  bool defer_too_many = false;
  DevBuf<float> d_pred;
  PinnedBuf<float> h_pred;
  // several output groups: the [G][nrow] margin planes the walks write and group_finish reads, and the [nrow][T] leaf
  // ids of a walk of all trees in group-major order with the map that puts them back in file order - buffers of the
  // booster's own, never a fields or Run1 one
  DevBuf<float> d_planes, d_gleaf;
  DevBuf<uint32_t> d_flat_of_file;
  // the library's two streams on the booster's device (lib_streams; not the booster's to destroy).  Host forms of the
  // fused calls: PCIe copies on s_copy beside the kernels on s_exec.  OH Run1's device form: the slab count, and the
  // streaming kernels of the pieces that are not being walked, on s_copy beside the caller's stream
  hipStream_t s_copy = nullptr, s_exec = nullptr;
  hipEvent_t run1_fork = nullptr, run1_slab = nullptr, run1_join = nullptr, run1_clear = nullptr;
  std::vector<hipEvent_t> run1_prep, run1_walk, run1_feed_events;
  // ohx_copy_engine = auto: the host form of Run1 on this booster decides by its own clock.  After two ticks of warm-up,
  // eight ticks of each engine in runs of four (K K K K D D D D K K K K D D D D); the lower median wins; every 512 ticks
  // the trial is run again (ranks come and go); a block of another size starts over.  Both engines give the same bits.
  struct CopyEngineTrial {
    size_t vol = 0;
    unsigned tick = 0;                 // since the trial (re)started
    int choice = -1;                   // -1 = trying
    unsigned trials = 0, picked_dma = 0;
    std::vector<double> seconds[2];
    static constexpr unsigned kWarm = 2, kRun = 4, kEach = 8, kAgain = 512;
    bool dma_now(size_t v) {
      if (v != vol) { vol = v; tick = 0; choice = -1; seconds[0].clear(); seconds[1].clear(); }
      if (choice >= 0 && tick >= kAgain) { tick = kWarm; choice = -1; seconds[0].clear(); seconds[1].clear(); }
      if (choice >= 0) return choice == 1;
      if (tick < kWarm) return false;
      return ((tick - kWarm) / kRun) % 2 == 1;
    }
    void report(bool dma, double s) {
      const unsigned t = tick++;
      if (choice >= 0 || t < kWarm) return;
      seconds[dma ? 1 : 0].push_back(s);
      if (seconds[0].size() >= kEach && seconds[1].size() >= kEach) {
        double med[2];
        for (int e = 0; e < 2; ++e) {
          std::sort(seconds[e].begin(), seconds[e].end());
          med[e] = seconds[e][seconds[e].size() / 2];
        }
        choice = med[1] < med[0] ? 1 : 0;
        ++trials;
        picked_dma += (unsigned)choice;
        if (getenv("OHX_DEBUG"))
          fprintf(stderr, "[libohxgb] copy engine trial %u on a block of %zu gridcells: median tick %.1f us by copy kernels, %.1f us by DMA -> %s\n",
                  trials, vol, med[0] * 1e6, med[1] * 1e6, choice ? "dma" : "kernel");
      }
    }
  } copy_trial;
  PinnedBuf<int32_t> h_slab;
  std::vector<DevBuf<float>> d_stage;  // fused host path: per-field staging
  DevBuf<float> d_stage_out, d_stage_margin;
  // Run1: engineered features, OH_ML and the slab result stay in HBM between the steps
  DevBuf<float> d_run1[10];
  DevBuf<int32_t> d_slab;
  bool slab_zeroed = false;            // d_slab's two words are zero whenever no slab count is enqueued (run1_device) ...
  hipStream_t slab_zeroed_on = nullptr; // ... by a memset on this stream, with run1_clear recorded behind it
  // clustering pass for rows in no known order (kernels.hip)
  DevBuf<uint32_t> d_cluster_keys[2], d_cluster_vals[2], d_cluster_small;
  DevBuf<uint8_t> d_cluster_temp;
  PinnedBuf<uint32_t> h_cluster_small;
  // the walk that reads the permutation out of the buffers above is asynchronous: recorded behind it, waited for by
  // the next clustering pass on this booster whatever stream that one runs on
  hipEvent_t cluster_done = nullptr;
  bool cluster_in_flight = false;
  std::vector<DevBuf<float>> d_run1_stage;
  // Categorical splits (docs/14_categorical.md): a booster that holds at least one is walked from a node format of
  // its own (flatten.hpp CatNode) by the kernels of categorical.hip and has none of the device forms above but the
  // roots; num_cat == 0 - every other booster - builds and launches exactly what it always did.
  uint64_t num_cat = 0;
  DevBuf<CatNode> d_cat_nodes;
  DevBuf<uint32_t> d_cat_words;
  DevBuf<int32_t> d_cat_orig;
  uint64_t cat_word_count = 0, cat_inline_sets = 0, cat_word_sets = 0;
  bool cat_force_direct = false;        // "ohx_cat_kernel" = direct: margins by the direct kernel too (same bits)
  std::unique_ptr<ContribsState> contribs;
  bool contribs_split = true;           // "ohx_contribs_split": small batches may have their trees split over waves
  std::unique_ptr<LeafWalkState> leaf_walk;   // shared by the two below; dropped only together with them
  std::unique_ptr<VisitState> visits;
  bool visits_use_lds = false;          // "ohx_visits_kernel" = lds: trees whose leaf histogram fits in LDS keep it there
                                        // (auto and global: every tree the global way - the faster at C360; same integers)
  uint32_t visits_lds_leaves = 0;       // "ohx_visits_lds_leaves": leaves a block's LDS histogram may hold (0 = what fits)
  // boosting (docs/26_objectives.md): kept on the handle, never written into a model file
  uint32_t grow_objective = kGrowObjSquared;   // "ohx_objective": squarederror, pseudohuber or quantile
  float grow_quantile_alpha = 0.5f;            // "ohx_quantile_alpha": alpha of the quantile objective and metric
  float grow_slope = 1.0f;                     // "ohx_huber_slope": delta of pseudohuber
  bool grow_pairs_on = false;                  // "ohx_grow_pairs" = on: squared error goes through the pair kernels too (same bits)
  // (docs/27_regularisation_and_metrics.md): likewise on the handle alone
  float grow_alpha = 0.0f;                     // "ohx_reg_alpha": the L1 threshold on a node's gradient sum
  float grow_max_delta_step = 0.0f;            // "ohx_max_delta_step": the bound on |base_weight|; 0 is off
  uint32_t grow_metric = kGrowMetricRmse;      // "ohx_eval_metric": what train_rmse[] / eval_rmse[] hold and the stop rule compares
  // (docs/28_monotone_constraints.md): "ohx_monotone_constraints", entry f is c_f; empty is the default, and a list of
  // zeros is kept as the empty list it stands for
  std::vector<int8_t> grow_mono;
  // (docs/29_colsample_level_node.md): "ohx_colsample_bylevel" and "ohx_colsample_bynode", the fraction of a tree's features a
  // level sees and of a level's a node does; 1 is the default
  float grow_bylevel = 1.0f, grow_bynode = 1.0f;
  // (docs/35_interaction_constraints.md): "ohx_interaction_constraints", the groups as two words of feature bits each; empty
  // is the default
  std::vector<uint64_t> grow_interact;
  std::unique_ptr<RefitState> refit;
  std::unique_ptr<GrowState> grow;
};

// the leaf walk with both states that refer to it
void drop_leaf_walk(BoosterObj& b) {
  b.visits.reset();
  b.refit.reset();
  b.leaf_walk.reset();
}

DMatrixObj* as_dmat(DMatrixHandle h) {
  if (h == nullptr || !g_dmats.has(h)) throw OhxError("DMatrix handle is invalid or has been freed");
  return static_cast<DMatrixObj*>(h);
}

// a matrix that names its device is walked by a booster on that device only
void check_same_device(const DMatrixObj& d, int ordinal) {
  if (d.device >= 0 && d.device != ordinal)
    throw OhxError("the DMatrix lives on HIP device " + std::to_string(d.device) + " but the booster on device " +
                   std::to_string(ordinal));
}

BoosterObj* as_booster(BoosterHandle h) {
  if (h == nullptr || !g_boosters.has(h)) throw OhxError("Booster handle is invalid or has been freed");
  return static_cast<BoosterObj*>(h);
}

// Tree tops (and the ring kernels) pay where the texture addresser is the bound: deep trees.  Measured on the MI355X
// with the OH recipe's boosters (profiles/r02_sweeps.txt): 9 steps per tree (depth 18) 3.4 % faster with tops, 5 steps
// (depth 10) 10 % slower, 3 steps (depth 6) 27 % slower.
constexpr double kTreeTopsMinMeanSteps = 7.0;
constexpr double kRingMinMeanSteps = 5.0;

KernelKind pick_kernel(const BoosterObj& b) {
  const std::string& k = b.kernel_name;
  if (k == "wide") return KernelKind::Wide;
  if (b.super_ok) {
    if (k == "super1") return KernelKind::Super1;
    if (k == "super3") return KernelKind::Super3;
    if (k == "super4") return KernelKind::Super4;
    // forests of some depth walk fastest with their tree tops resident in LDS (kernels.hip, the ring kernels), against
    // the tile kernel: 9 steps per tree (the OH booster, depth 18) -20 %, 7 steps -16 %, 6 steps -6 %, 5 steps -3 %,
    // 4 steps +2 %, 3 steps +29 % (profiles/r04_sweeps.txt)
    if (k == "ring" || (k == "auto" && b.forest.num_feature == 27 && b.super_mean_steps >= kRingMinMeanSteps))
      return KernelKind::Ring;
    if (k == "super2" || k == "auto") return KernelKind::Super2;
  }
  if (!b.packed_ok) return KernelKind::Wide;
  if (k == "packed1") return KernelKind::Packed1;
  if (k == "packed4") return KernelKind::Packed4;
  return KernelKind::Packed2;
}

// Vector-memory instructions a wave issues to walk the whole forest once (walk_super).  With tree tops: per tree
// one coalesced load of its top (steps 1-3) and one gather for every step after the third, of at least four
// steps.  Without: a gather per step, less the first step of the trees whose start nodes sit in the kernels'
// LDS table.
uint64_t count_super_gathers(const SuperForest& sf, int mode) {   // 0 plain walk, 1 tree tops, 2 ring kernels
  uint64_t n = 0;
  for (size_t t = 0; t < sf.heads.size(); ++t) {
    const uint32_t steps = sf.heads[t].steps;
    if (mode == 2) n += (steps < 4u ? 4u : steps) - 4u;        // steps 1-4 from LDS
    else n += mode == 1 ? (steps < 4u ? 4u : steps) - 2u : steps - (t < kFirstStepTrees && steps ? 1u : 0u);
  }
  // ring: a group of four trees is staged with 11 wave loads, once per block of 16 waves
  if (mode == 2) n += (sf.heads.size() * 11 + 63) / 64;
  return n;
}

double mean_super_steps(const SuperForest& sf) {
  double n = 0;
  for (const SuperTreeHead& h : sf.heads) n += h.steps;
  return sf.heads.empty() ? 0.0 : n / (double)sf.heads.size();
}
bool use_tree_tops(const LaunchTuning& tune, double mean_steps) {
  return tune.tree_tops < 0 ? mean_steps >= kTreeTopsMinMeanSteps : tune.tree_tops != 0;
}

// the kind an "ohx_kernel" name stands for ("auto" is none: pick_kernel decides by the booster)
bool kind_of_name(const std::string& k, KernelKind* out) {
  for (KernelKind c : {KernelKind::Wide, KernelKind::Packed1, KernelKind::Packed2, KernelKind::Packed4, KernelKind::Super1,
                       KernelKind::Super2, KernelKind::Super3, KernelKind::Super4, KernelKind::Ring})
    if (k == kernel_kind_name(c)) {
      *out = c;
      return true;
    }
  return false;
}

bool wants_super(const std::string& k) {
  KernelKind kind;
  return k == "auto" || (kind_of_name(k, &kind) && kind_is_super(kind));
}

void invalidate_device_state(BoosterObj& b) {
  b.uploaded = false;
  b.d_packed.release();
  b.d_wide.release();
  b.d_super.release();
  b.d_super_heads.release();
  b.super_ok = false;
  b.d_roots.release();
  b.d_flat_of_file.release();
  b.d_cat_nodes.release();
  b.d_cat_words.release();
  b.d_cat_orig.release();
}

void ensure_wide(BoosterObj& b) {
  if (b.d_wide.p) return;
  std::vector<WideNode> wide = emit_wide(b.flat(), b.placement);
  b.d_wide.upload(wide);
}

void ensure_train_stream(BoosterObj& b);

void ensure_uploaded(BoosterObj& b) {
  if (!b.loaded) throw OhxError("the booster holds no model: call XGBoosterLoadModel first");
  if (b.uploaded) {
    HIP_CHECK(hipSetDevice(b.dev.ordinal));
    return;
  }
  b.dev = use_device(b.device_pref);
  const Forest& flat = b.flat();
  b.placement = place_forest(flat, b.layout);
  b.packed_ok = packed_format_fits(flat, b.placement);
  b.d_roots.upload(b.placement.roots);
  if (b.num_cat != 0) {
    // categorical splits: the one format the kernels of categorical.hip read, whatever ohx_kernel says
    CatForest cf = emit_cat(flat, b.placement);
    b.cat_word_count = cf.words.size();
    b.cat_inline_sets = cf.inline_sets;
    b.cat_word_sets = cf.word_sets;
    if (cf.words.empty()) cf.words.push_back(0u);
    b.d_cat_nodes.upload(cf.nodes);
    b.d_cat_words.upload(cf.words);
    b.d_cat_orig.upload(cf.orig_id);
  } else if (wants_super(b.kernel_name)) {
    SuperForest sf;
    b.super_ok = emit_super(flat, &sf, b.layout.super_pack) && sf.nodes.size() * sizeof(SuperNode) < 0xFFFFFFF0ull;
    if (b.super_ok) {
      b.super_slots = sf.nodes.size();
      b.super_gathers[0] = count_super_gathers(sf, 0);
      b.super_gathers[1] = count_super_gathers(sf, 1);
      b.super_gathers[2] = count_super_gathers(sf, 2);
      b.super_mean_steps = mean_super_steps(sf);
      b.d_super.upload(sf.nodes);
      // groups 2k and 2k + 1 of a tree are one cache line (flatten.hpp kSuperPack*) only in an array that starts on one
      if (((uintptr_t)b.d_super.p & 127u) != 0) throw OhxError("internal error: the super-node array is not 128-byte aligned");
      b.d_super_heads.upload(sf.heads);
    }
  }
  if (b.num_cat == 0 && b.packed_ok && !(b.super_ok && wants_super(b.kernel_name))) {
    std::vector<PackedNode> packed = emit_packed(flat, b.placement, nullptr);
    b.d_packed.upload(packed);
  }
  if (b.num_cat == 0 && pick_kernel(b) == KernelKind::Wide) ensure_wide(b);
  b.d_flags.ensure(3);      // [0] kFlag* bits, [1] ring re-runs counted on the device, [2] the train a block last gave up in
  {
    LibStreams& ls = lib_streams(b.dev.ordinal);
    b.s_exec = ls.exec;
    b.s_copy = ls.copy;
  }
  HIP_CHECK(hipMemsetAsync(b.d_flags.p, 0, 3 * sizeof(uint32_t), b.s_exec));
  HIP_CHECK(hipStreamSynchronize(b.s_exec));
  b.ring_reruns_seen = 0;
  ensure_train_stream(b);
  b.uploaded = true;
}

// the launch train's second stream exists only for a booster that was told to use it (ohx_overlap_group >= 2: an
// experiment knob): a stream is a hardware queue for the life of the process (LibStreams)
void ensure_train_stream(BoosterObj& b) {
  b.tune.train = nullptr;
  if (b.tune.overlap_group < 2) return;
  if (!b.train.side) {
    HIP_CHECK(hipStreamCreateWithFlags(&b.train.side, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&b.train.fork, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&b.train.join, hipEventDisableTiming));
  }
  b.tune.train = &b.train;
}

DeviceForest device_forest(const BoosterObj& b) {
  DeviceForest d;
  d.packed = b.d_packed.p;
  d.wide = b.d_wide.p;
  d.roots = b.d_roots.p;
  d.super = b.d_super.p;
  d.super_heads = b.d_super_heads.p;
  d.packed_bytes = (uint32_t)(b.d_packed.n * sizeof(PackedNode));
  d.super_bytes = (uint32_t)(b.d_super.n * sizeof(SuperNode));
  d.num_trees = (uint32_t)b.forest.trees.size();
  d.num_feature = b.forest.num_feature;
  d.base_score = b.margin_base;
  d.tree_tops = (b.super_ok && use_tree_tops(b.tune, b.super_mean_steps)) ? 1u : 0u;
  return d;
}

void tree_range(const BoosterObj& b, unsigned ntree_limit, uint32_t* t0, uint32_t* t1) {
  const uint32_t T = (uint32_t)b.forest.trees.size();
  *t0 = 0;
  *t1 = (ntree_limit == 0 || ntree_limit > T) ? T : ntree_limit;
}

// `finish`: what group_finish makes of the margins of a booster with several output groups (groups.hpp)
void check_predict_options(const BoosterObj& b, int option_mask, bool* pred_leaf, int* finish = nullptr) {
  *pred_leaf = false;
  if (finish) *finish = kGroupMargins;
  if (option_mask == 0 || option_mask == 1) {
    if (!b.margin_error.empty()) throw OhxError(b.margin_error);
    // the two multi-class transforms, for boosters of several output groups (a single group keeps the refusal below)
    if (option_mask == 0 && finish && b.num_groups >= 2 &&
        (b.forest.objective == "multi:softprob" || b.forest.objective == "multi:softmax")) {
      *finish = b.forest.objective == "multi:softprob" ? kGroupSoftprob : kGroupArgmax;
      return;
    }
    if (option_mask == 0 && !objective_is_identity(b.forest.objective))
      throw OhxError("objective '" + b.forest.objective +
                     "' needs a prediction transform this library does not implement; "
                     "use option_mask = 1 (margin) or a reg:squarederror model");
    return;
  }
  if (option_mask == 16) {
    *pred_leaf = true;
    return;
  }
  throw OhxError("XGBoosterPredict: option_mask " + std::to_string(option_mask) +
                 " is not supported (0 = value, 1 = margin, 16 = leaf index)");
}

// Several output groups.  ntree_limit = k > 0 means the first k rounds: file trees [0, min(T, k * G)) (xgboost 1.6.0's
// GetIterationFromTreeLimit with num_parallel_tree = 1); 0 means all trees.
uint32_t group_tree_limit(const BoosterObj& b, unsigned ntree_limit) {
  const uint64_t T = b.forest.trees.size(), want = (uint64_t)ntree_limit * b.num_groups;
  return (uint32_t)((ntree_limit == 0 || want > T) ? T : want);
}
// ... and each group's share of file trees [0, L): a prefix of the group's range in the group-major copy, whose trees
// keep their file order
std::vector<uint32_t> group_tree_counts(const BoosterObj& b, uint32_t L) {
  std::vector<uint32_t> n(b.num_groups, 0u);
  for (uint32_t t = 0; t < L; ++t) ++n[(size_t)b.forest.tree_info[t]];
  return n;
}
// floats XGBoosterPredict returns for a booster of several output groups
size_t group_predict_len(const BoosterObj& b, uint64_t nrow, int option_mask, unsigned ntree_limit) {
  if (option_mask == 16) return (size_t)nrow * group_tree_limit(b, ntree_limit);
  if (option_mask == 0 && b.forest.objective == "multi:softmax") return (size_t)nrow;
  return (size_t)nrow * b.num_groups;
}
// The OH shell's forms (fields, contributions from the fields, Run1) are single-output
void refuse_groups(const BoosterObj& b, const char* what) {
  if (b.loaded && b.num_groups >= 2)
    throw OhxError(std::string(what) + " is single-output: this booster has " + std::to_string(b.num_groups) +
                   " output groups (multi-class or multi-target); predict it through XGBoosterPredict or "
                   "OHXBoosterPredictDevice");
}

// What a booster with categorical splits cannot do yet is refused at the top of the call, before an argument is read
// or the device is touched (include/ohxgb.h part 5)
void refuse_categorical(const BoosterObj& b, const char* what) {
  if (b.loaded && b.num_cat != 0)
    throw OhxError(std::string(what) + " does not take a booster with categorical splits (this one has " +
                   std::to_string(b.num_cat) + "); predict it through XGBoosterPredict or OHXBoosterPredictDevice");
}

DeviceCatForest device_cat_forest(const BoosterObj& b) {
  DeviceCatForest d;
  d.nodes = b.d_cat_nodes.p;
  d.node_bytes = (uint32_t)(b.d_cat_nodes.n * sizeof(CatNode));
  d.words = b.d_cat_words.p;
  d.orig_id = b.d_cat_orig.p;
  d.roots = b.d_roots.p;
  d.num_trees = (uint32_t)b.forest.trees.size();
  d.num_feature = b.forest.num_feature;
  d.base_score = b.margin_base;
  return d;
}

void check_columns(const BoosterObj& b, uint64_t ncol) {
  if (ncol > b.forest.num_feature)
    throw OhxError("Number of columns does not match number of features in booster (" + std::to_string(ncol) +
                   " vs. " + std::to_string(b.forest.num_feature) + ")");
}

void judge_flags(BoosterObj& b, const uint32_t flags[2], hipStream_t stream);

void raise_flag_errors(BoosterObj& b, hipStream_t stream) {
  uint32_t flags[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(flags, b.d_flags.p, sizeof(flags), hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  judge_flags(b, flags, stream);
}

// `flags` = the first two words of d_flags as read back behind the work on `stream`, which the caller has waited for
void judge_flags(BoosterObj& b, const uint32_t flags[2], hipStream_t stream) {
  // a ring block that timed out is not an error: its rows were walked again by the tile kernel on the stream, behind
  // the train (kernels.hip launch_ring_rerun); worth a line on stderr the first time, and a counter from then on
  if (flags[1] != b.ring_reruns_seen) {
    if (b.ring_reruns_seen == 0)
      fprintf(stderr, "[libohxgb] warning: a block of the ring kernel gave up waiting for another; the batch was predicted "
                      "again by the tile kernel (same results, slower).  Counted in OHXBoosterRingReruns; "
                      "ohx_kernel=super2 avoids the ring kernels.\n");
    b.ring_reruns_seen = flags[1];
  }
  if (flags[0] != 0) {
    HIP_CHECK(hipMemsetAsync(b.d_flags.p, 0, sizeof(uint32_t), stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (flags[0] & kFlagInfInput) throw OhxError("Input data contains `inf` or `nan`");
    throw OhxError("the predict kernel reported error flags " + std::to_string(flags[0]));
  }
}

// A parsed model becomes the booster's: what the readers forgave goes to stderr (as xgboost's LOG(WARNING)
// does), the margin every prediction starts from is fixed here.
void adopt_model(BoosterObj& b, Forest&& f) {
  f.validate();
  for (const std::string& w : f.warnings) fprintf(stderr, "[libohxgb] warning: model file: %s\n", w.c_str());
  invalidate_device_state(b);
  b.contribs.reset();
  drop_leaf_walk(b);
  b.grow.reset();
  b.forest = std::move(f);
  b.num_groups = b.forest.num_groups();
  b.num_cat = b.forest.num_categorical_splits();
  b.grouped = Forest();
  b.group_begin.clear();
  b.flat_file_index.clear();
  if (b.num_groups >= 2) b.grouped = group_major(b.forest, &b.group_begin, &b.flat_file_index);
  b.loaded = true;
  b.margin_error.clear();
  try {
    b.margin_base = b.forest.margin_base();
  } catch (const OhxError& e) {
    b.margin_base = b.forest.base_score;
    b.margin_error = e.what();       // leaf indices (option_mask 16) still work
  }
}

bool ends_with(const std::string& s, const std::string& suf) {
  return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0;
}

// A caller that does not say which grid its rows were gathered from (OHXDMatrixSetGrid) - the
// reference's own call sequence - still shows the size of a level: the gather stacks levels
// (OH_GridCompMod.F90:309-345) and its first column is a 2-D field (LAT, :313), so that column repeats
// bit for bit with the level size as period.  Knowing the level size alone the kernels take runs of
// 8 cells x 8 levels per wave, which measures within 1 % of the full 4x4x4 bricks (34.8 vs 34.6 ms per
// C360 step; 40.9 ms without).  Speed only: any period gives a valid tiling of the rows.
// The search runs once per matrix, at its first predict (or OHXDMatrixGetGrid / OHXDMatrixInferGrid), and
// not at all when the caller has named the grid by then (OHXDMatrixSetGrid).
constexpr uint64_t kMinLevel = 4096, kMaxLevels = 1024;

uint32_t level_candidates(const DMatrixObj& d) {
  if (d.ncol < 1 || d.nrow < 2 * kMinLevel) return 0;
  return (uint32_t)std::min<uint64_t>(kMaxLevels, d.nrow / kMinLevel);       // kmax: candidates k = kmax .. 2
}

// LAT is the first column of the OH gather; the last one (SZA) and the 2-D fields in between
// (GMISTRATO3, ALBUV, :334-335) serve a caller whose first column is something else
PeriodColumns level_columns(const DMatrixObj& d) { return PeriodColumns{{0u, (uint32_t)d.ncol - 1u, 21u, 22u}}; }

// verdict[c * (kmax - 1) + x]: 0 = column c repeats with period nrow / (kmax - x)
void adopt_level_size(DMatrixObj& d, const uint32_t* verdict, uint32_t kmax) {
  d.grid_looked = true;
  const uint64_t period = pick_level_period(verdict, kmax, d.nrow);      // kernels.hpp: column order, then the smallest
  if (period == 0) return;
  d.grid_im = (int)period;
  d.grid_jm = 1;
  d.grid_row0 = 0;
  d.grid_inferred = true;
}

// What the search found for matrices of a shape seen before.  The reference creates and frees its DMatrix on every
// OH tick (OH_GridCompMod.F90:347,377) with the same N x 27 every time: the launches and the host wait of the search
// are paid at the first tick only.  Speed only - any period is a valid tiling of the rows - so a later matrix of the
// same shape from another grid is tiled with the remembered level size, not wrongly.  OHXDMatrixInferGrid always looks.
struct LevelSizeCache {
  std::mutex mu;
  struct Entry {
    uint64_t nrow, ncol;
    int period;      // 0 = looked and found none
    unsigned hits;   // since the last real search
  };
  std::vector<Entry> seen;
  // A verdict - either way - is only taken on trust fifteen times in a row; the sixteenth matrix of the shape is
  // searched again (one read-back), so that one odd matrix - shuffled rows, a constant first column - cannot decide
  // how every later matrix of its shape is tiled for the life of the process.
  bool find(uint64_t nrow, uint64_t ncol, int* period) {
    std::lock_guard<std::mutex> g(mu);
    for (Entry& e : seen)
      if (e.nrow == nrow && e.ncol == ncol) {
        if (++e.hits >= 16) return false;
        *period = e.period;
        return true;
      }
    return false;
  }
  void put(uint64_t nrow, uint64_t ncol, int period) {
    std::lock_guard<std::mutex> g(mu);
    for (Entry& e : seen)
      if (e.nrow == nrow && e.ncol == ncol) {
        e.period = period;
        e.hits = 0;
        return;
      }
    if (seen.size() >= 64) seen.erase(seen.begin());
    seen.push_back({nrow, ncol, period, 0u});
  }
};
LevelSizeCache g_level_sizes;

bool stream_capturing(hipStream_t stream);                 // defined with the deferred rows below
[[noreturn]] void refuse_in_capture(const char* what, const char* advice = nullptr);

// Launches + one read-back on `stream`; waits for it (the rows must be there) - unless a matrix of this shape has
// been searched before and `use_cache` allows taking its verdict.
void infer_level_size(DMatrixObj& d, hipStream_t stream, bool use_cache = false) {
  d.grid_looked = true;
  const uint32_t kmax = level_candidates(d);
  if (kmax < 2) return;
  int period = 0;
  if (use_cache && g_level_sizes.find(d.nrow, d.ncol, &period)) {
    if (period > 0) {
      d.grid_im = period;
      d.grid_jm = 1;
      d.grid_row0 = 0;
      d.grid_inferred = true;
    }
    return;
  }
  {
    std::lock_guard<std::mutex> g(g_check.mu);
    const size_t words = (size_t)4 * (kmax - 1);
    g_check.ensure(words, d.device);
    HIP_CHECK(hipMemsetAsync(g_check.d.p, 0, words * sizeof(uint32_t), stream));
    HIP_CHECK(launch_detect_period(d.d_data, d.nrow, (uint32_t)d.ncol, level_columns(d), 4, kmax, g_check.d.p, stream));
    HIP_CHECK(hipMemcpyAsync(g_check.h.p, g_check.d.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    adopt_level_size(d, g_check.h.p, kmax);
  }
  g_level_sizes.put(d.nrow, d.ncol, d.grid_inferred ? d.grid_im : 0);
}

// Rows nobody has described and in which no level size was found: group them by the decisions they take at
// the top of the booster's first trees (kernels.hip) and let every wave take 64 rows of one group.  Returns the
// permutation to walk through, or nullptr for "as they come".  Judged once per matrix (one wait on the stream,
// like the level-size search): rows that mostly agree with their predecessor are in some useful order already.
const uint32_t* cluster_rows(BoosterObj& b, DMatrixObj& d, const PredictArgs& a, bool pred_leaf, KernelKind kind,
                             hipStream_t stream) {
  constexpr uint64_t kMinRows = 1u << 18;
  if (b.tune.cluster == 0 || pred_leaf || d.grid_im != 0 || !b.super_ok || kind == KernelKind::Wide) return nullptr;
  if (d.nrow > 0xFFFFFFF0ull || d.ncol > b.forest.num_feature || b.forest.num_feature > 32) return nullptr;
  if (b.tune.cluster < 0 && (d.nrow < kMinRows || (d.cluster_decided && !d.cluster_on))) return nullptr;
  ClusterArgs c;
  c.rows = d.d_data;
  c.nrow = d.nrow;
  c.ncol = (uint32_t)d.ncol;
  c.missing = d.missing;
  c.ntrees = (uint32_t)std::min<size_t>((size_t)std::max(b.tune.cluster_trees, 1), b.forest.trees.size());
  c.nsteps = (uint32_t)std::max(b.tune.cluster_steps, 1);
  c.zorder = b.tune.cluster_zorder ? 1u : 0u;
  c.ntrees = std::min<uint32_t>(c.ntrees, 4u);
  while (cluster_key_bits(c) > 32u && c.nsteps > 1) --c.nsteps;
  while (cluster_key_bits(c) > 32u && c.ntrees > 1) --c.ntrees;
  const unsigned sort_bits = cluster_key_bits(c);
  // an earlier walk of this booster may still be reading its permutation out of these buffers (another stream,
  // another matrix): the keys of this pass go in behind it
  if (b.cluster_in_flight) HIP_CHECK(hipStreamWaitEvent(stream, b.cluster_done, 0));
  for (int q = 0; q < 2; ++q) {
    b.d_cluster_keys[q].ensure(d.nrow);
    b.d_cluster_vals[q].ensure(d.nrow);
  }
  b.d_cluster_small.ensure(9);
  b.h_cluster_small.ensure(9);
  c.keys = b.d_cluster_keys[0].p;
  c.vals = b.d_cluster_vals[0].p;
  c.agree = b.d_cluster_small.p;
  HIP_CHECK(hipMemsetAsync(c.agree, 0, 9 * sizeof(uint32_t), stream));
  HIP_CHECK(launch_cluster_keys(device_forest(b), c, b.dev.num_cus, stream));
  if (b.tune.cluster < 0 && !d.cluster_decided) {
    if (stream_capturing(stream)) refuse_in_capture("judge the order of the rows (it waits for the stream)");
    HIP_CHECK(hipMemcpyAsync(b.h_cluster_small.p, c.agree, 9 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    // observed agreement between neighbours in row order against what rows in random order would show
    // (sum of squared shares of the eight outcomes): 0 = as good as shuffled, 1 = every row like the one before
    double observed = 0.0, by_chance = 0.0;
    const double order = cluster_order(b.h_cluster_small.p, d.nrow, &observed, &by_chance);      // kernels.hpp
    d.cluster_decided = true;
    d.cluster_on = order < kClusterOrderBelow;
    if (getenv("OHX_DEBUG"))
      fprintf(stderr, "[libohxgb] cluster verdict: %.1f %% of the rows take the first three decisions of the row before them, "
              "%.1f %% would by chance: order %.2f -> %s\n", 100.0 * observed, 100.0 * by_chance, order,
              d.cluster_on ? "cluster" : "leave");
    if (!d.cluster_on) return nullptr;
  }
  size_t temp_bytes = 0;
  HIP_CHECK(sort_pairs_u32(nullptr, &temp_bytes, c.keys, b.d_cluster_keys[1].p, c.vals, b.d_cluster_vals[1].p, d.nrow,
                           sort_bits, stream, nullptr));
  b.d_cluster_temp.ensure(temp_bytes);
  uint32_t* sorted = nullptr;
  HIP_CHECK(sort_pairs_u32(b.d_cluster_temp.p, &temp_bytes, c.keys, b.d_cluster_keys[1].p, c.vals, b.d_cluster_vals[1].p,
                           d.nrow, sort_bits, stream, &sorted));
  return sorted;
}

// Deferred rows (kernels.hpp PredictArgs::defer_list).  The second launch pays while few rows hold missing values
// (1e-4 of the entries: +2 % instead of +17 %); from about one row in fifty on it costs what it saves, and more beyond
// (profiles/r03_sweeps.txt).  The count of the last batch - read back behind it, never waited for - decides; the
// reference's ticks resemble each other.  Returns whether the launch will count (and maybe list) such rows.
// A small batch or slab: room for the leaves of its trees, so that they can be walked by several waves per tile
// (kernels.hpp PredictArgs::leaf_buf; only batches that can qualify: their tiles fill at most half of the chip's 20
// waves per CU).
// `im`, `jm`, `row0`: the grid the rows come from (0 = unknown): the buffer is sized for the tiles the launcher will
// really make of them - bricks over the rows' levels, or 64 consecutive rows where bricks would be mostly empty -
// not for a bound (a 48 x 24 x 72 rank block took 73 MB per booster; now 24 MB).
// `plan_only` (OHXBoosterKernelSymbolRows, a query): what a predict of this batch WOULD be handed - the buffer as it is or
// as it would be made - without making it: the launch planner only looks at the pointer being non-NULL and at the size.
float* const kPlannedBuffer = reinterpret_cast<float*>((uintptr_t)256);
void leaf_room(BoosterObj& b, uint64_t nrow, uint32_t ntree, LaunchTuning& tune, int im, int jm, uint64_t row0,
               bool plan_only = false) {
  if (tune.tree_split == 0 || !b.super_ok || nrow == 0 || nrow > (uint64_t)b.dev.num_cus * 10u * 64u + 4096u) return;
  // the launcher's shape (kernels.hpp pick_shape), or the consecutive rows it falls back to, whichever makes more tiles
  const size_t tiles = (size_t)std::max(TileShape().ntiles(nrow), pick_shape(tune, im, jm, row0, nrow).ntiles(nrow));
  if (plan_only) {
    tune.leaf_buf = b.d_leaves.p != nullptr ? b.d_leaves.p : kPlannedBuffer;
    tune.leaf_words = std::max(b.d_leaves.n, tiles * 64 * (size_t)ntree);
    return;
  }
  b.d_leaves.ensure(tiles * 64 * (size_t)ntree);
  tune.leaf_buf = b.d_leaves.p;
  tune.leaf_words = b.d_leaves.n;
}

// What defer_prepare would say and hand out for this batch, touching nothing: not the pending read-back, not
// defer_too_many, no allocation, no memset on any stream (the query used to do all four, the memset on NULL).
bool defer_plan(const BoosterObj& b, uint64_t nrow, LaunchTuning& tune) {
  if (!DeferRule::wanted(tune, nrow)) return false;
  tune.defer_buf = b.d_defer.p != nullptr ? b.d_defer.p : reinterpret_cast<uint32_t*>(kPlannedBuffer);
  tune.defer_words = std::max(b.d_defer.n, (size_t)DeferRule::defer_capacity(nrow) + 1);
  tune.defer_count_only = (b.defer_too_many && tune.defer_missing < 0) ? 1 : 0;
  return true;
}

// Is `stream` being captured into a hipGraph?  The device forms (OHXBoosterPredictDevice, OHXBoosterPredictFieldsDevice)
// may be: what they enqueue is launches, memsets and copies on the caller's stream and nothing else, once the
// booster's buffers exist and the matrix has been looked at - i.e. after one plain call of the same shape.  What the
// host does BESIDE the launches to adapt the next call (the read-back of how many rows were left to the second launch,
// the event query that consumes it) is left out while capturing: a replay could not repeat it, and an event query is
// not allowed beside a capture.  The captured work is what the last plain call decided.
bool stream_capturing(hipStream_t stream) {
  if (stream == nullptr) return false;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &st) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return st == hipStreamCaptureStatusActive;
}

[[noreturn]] void refuse_in_capture(const char* what, const char* advice) {
  throw OhxError(std::string("inside a stream capture the library cannot ") + what + ": " +
                 (advice ? advice : "make one plain call of the same shape on this booster and matrix first, then capture"));
}

bool defer_prepare(BoosterObj& b, uint64_t nrow, LaunchTuning& tune, hipStream_t stream) {
  if (!DeferRule::wanted(tune, nrow)) return false;
  const size_t words = (size_t)DeferRule::defer_capacity(nrow) + 1;      // the count, then the list
  const bool capturing = stream_capturing(stream);
  if (!capturing && b.defer_pending && hipEventQuery(b.defer_seen) == hipSuccess) {
    b.defer_pending = false;
    b.defer_too_many = (uint64_t)b.h_defer_count.p[0] * 50u > b.defer_last_nrow;        // more than 2 % of the rows
  }
  const uint32_t* before = b.d_defer.p;
  if (capturing && b.d_defer.n < words) refuse_in_capture("allocate the list of rows left to the second launch");
  b.d_defer.ensure(words);
  // the launchers zero the count only when they really defer (kernels.hip launch_predict: prefetch kernel, no split
  // ...); defer_look reads it back regardless, so a buffer fresh from hipMalloc must not hold garbage
  // on the stream the launches and defer_look's read-back run on: those streams are non-blocking, a NULL-stream memset
  // is not ordered before them
  if (b.d_defer.p != before) HIP_CHECK(hipMemsetAsync(b.d_defer.p, 0, sizeof(uint32_t), stream));
  tune.defer_buf = b.d_defer.p;
  tune.defer_words = b.d_defer.n;
  tune.defer_count_only = (b.defer_too_many && tune.defer_missing < 0) ? 1 : 0;
  return true;
}

void defer_look(BoosterObj& b, uint64_t nrow, hipStream_t stream) {
  if (b.defer_pending || stream_capturing(stream)) return;
  if (b.defer_seen == nullptr) HIP_CHECK(hipEventCreateWithFlags(&b.defer_seen, hipEventDisableTiming));
  b.h_defer_count.ensure(1);
  HIP_CHECK(hipMemcpyAsync(b.h_defer_count.p, b.d_defer.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipEventRecord(b.defer_seen, stream));
  b.defer_pending = true;
  b.defer_last_nrow = nrow;
}

// A walk with what the booster lends it: room for the leaves of a small batch (`room`) and the list of the rows left to a
// second launch (`may_defer`), then `launch(tune)`, then the look at how many rows were listed.  `im`, `jm`, `row0`: as leaf_room.
template <class Launch>
void walk_with_buffers(BoosterObj& b, uint64_t nrow, uint32_t ntree, LaunchTuning tune, int im, int jm, uint64_t row0, bool room,
                       bool may_defer, hipStream_t stream, Launch launch) {
  if (room) leaf_room(b, nrow, ntree, tune, im, jm, row0);
  const bool deferring = may_defer && defer_prepare(b, nrow, tune, stream);
  HIP_CHECK(launch(tune));
  if (deferring) defer_look(b, nrow, stream);
}

// the booster's knobs and the grid the matrix's rows come from (kernels.hpp LaunchTuning::grid_im)
LaunchTuning tune_for(const BoosterObj& b, const DMatrixObj& d) {
  LaunchTuning tune = b.tune;
  tune.grid_im = d.grid_im;
  tune.grid_jm = d.grid_jm;
  tune.grid_row0 = d.grid_row0;
  return tune;
}

void launch_predict_groups(BoosterObj& b, DMatrixObj& d, int option_mask, unsigned ntree_limit, float* d_out,
                           hipStream_t stream);

// behind a walk that reads cluster_rows' permutation: what the next clustering pass on this booster waits for
void mark_cluster_in_flight(BoosterObj& b, hipStream_t stream) {
  if (b.cluster_done == nullptr) HIP_CHECK(hipEventCreateWithFlags(&b.cluster_done, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(b.cluster_done, stream));
  b.cluster_in_flight = true;
}

void launch_predict_checked(BoosterObj& b, DMatrixObj& d, int option_mask, unsigned ntree_limit, float* d_out,
                            hipStream_t stream) {
  if (b.loaded && b.num_groups >= 2) return launch_predict_groups(b, d, option_mask, ntree_limit, d_out, stream);
  bool pred_leaf = false;
  check_predict_options(b, option_mask, &pred_leaf);
  check_columns(b, d.ncol);
  if (b.loaded && b.num_cat != 0 && stream_capturing(stream))
    refuse_in_capture("predict a booster with categorical splits",
                      "its kernels are not among what a capture may hold yet; call it outside the capture");
  ensure_uploaded(b);
  check_same_device(d, b.dev.ordinal);
  if (b.num_cat != 0) {
    // the kernels of categorical.hip; of the launch knobs only the rows' grid and the brick shape apply (ohx_kernel, tree
    // split, deferred rows, the clustering pass and the level-size search do not)
    CatPredictArgs c;
    c.rows = d.d_data;
    c.nrow = d.nrow;
    c.ncol = (uint32_t)d.ncol;
    c.missing = d.missing;
    tree_range(b, ntree_limit, &c.tree_begin, &c.tree_end);
    c.out = d_out;
    c.pred_leaf = pred_leaf;
    c.flags = b.d_flags.p;
    HIP_CHECK(launch_predict_cat(device_cat_forest(b), c, b.dev.num_cus, b.cat_force_direct, stream, tune_for(b, d)));
    return;
  }
  KernelKind kind = pick_kernel(b);
  // nobody has said which grid the rows come from: look once (work on `stream` enqueued so far is waited for)
  // (a matrix the library copied itself - the reference's create / predict / free per tick - takes the verdict of
  // the last matrix of its shape instead of looking again)
  if (!d.grid_looked && d.grid_im == 0 && !pred_leaf && kind != KernelKind::Wide) {
    if (stream_capturing(stream)) refuse_in_capture("look for the rows' level size (it waits for the stream)");
    infer_level_size(d, stream, d.owned != nullptr);
  }
  if (pred_leaf || kind == KernelKind::Wide) ensure_wide(b);
  PredictArgs a;
  a.rows = d.d_data;
  a.nrow = d.nrow;
  a.ncol = (uint32_t)d.ncol;
  a.missing = d.missing;
  tree_range(b, ntree_limit, &a.tree_begin, &a.tree_end);
  a.out = d_out;
  a.pred_leaf = pred_leaf;
  a.flags = b.d_flags.p;
  a.perm = cluster_rows(b, d, a, pred_leaf, kind, stream);
  // rows with missing values leave for a second, small launch instead of slowing their whole wave down (big batches)
  const bool own_order = !pred_leaf && a.perm == nullptr;
  walk_with_buffers(b, d.nrow, a.tree_end - a.tree_begin, tune_for(b, d), d.grid_im, d.grid_jm, d.grid_row0, own_order,
                    own_order && d.ncol == 27, stream, [&](const LaunchTuning& tune) {
                      return launch_predict(kind, device_forest(b), a, b.dev.num_cus, stream, tune);
                    });
  if (a.perm != nullptr) mark_cluster_in_flight(b, stream);
}

// A booster of several output groups (docs/13_output_groups.md): each group's tree range is walked by the kernel the
// booster would pick anyway - ring, tiles with trees split over waves, deferred rows, the clustering pass - into its
// plane of [G][nrow] margins, exactly as a single-group booster of those trees is walked; a group without trees in the
// range is not walked and its plane holds the base margin.  group_finish then writes the output from the planes.  Leaf
// ids: all trees of the group-major copy are walked into [nrow][T] and gathered back to file order.  Not capturable:
// refused before anything is enqueued.
void launch_predict_groups(BoosterObj& b, DMatrixObj& d, int option_mask, unsigned ntree_limit, float* d_out,
                           hipStream_t stream) {
  bool pred_leaf = false;
  int finish = kGroupMargins;
  check_predict_options(b, option_mask, &pred_leaf, &finish);
  check_columns(b, d.ncol);
  if (stream_capturing(stream))
    refuse_in_capture("predict a booster of several output groups",
                      "its predict waits for the stream and fills the booster's own group planes; call it outside the capture");
  ensure_uploaded(b);
  check_same_device(d, b.dev.ordinal);
  const uint32_t G = b.num_groups, T = (uint32_t)b.forest.trees.size();
  const uint32_t L = group_tree_limit(b, ntree_limit);
  const uint64_t n = d.nrow;
  KernelKind kind = pick_kernel(b);
  if (!d.grid_looked && d.grid_im == 0 && !pred_leaf && kind != KernelKind::Wide) infer_level_size(d, stream, d.owned != nullptr);
  if (pred_leaf || kind == KernelKind::Wide) ensure_wide(b);
  PredictArgs a;
  a.rows = d.d_data;
  a.nrow = n;
  a.ncol = (uint32_t)d.ncol;
  a.missing = d.missing;
  a.flags = b.d_flags.p;
  LaunchTuning tune = tune_for(b, d);
  if (pred_leaf) {
    if (b.d_flat_of_file.p == nullptr && T != 0) {
      std::vector<uint32_t> flat_of_file(T);
      for (uint32_t i = 0; i < T; ++i) flat_of_file[b.flat_file_index[i]] = i;
      b.d_flat_of_file.upload(flat_of_file);
    }
    b.d_gleaf.ensure((size_t)n * T);
    a.tree_begin = 0;
    a.tree_end = T;
    a.out = b.d_gleaf.p;
    a.pred_leaf = true;
    HIP_CHECK(launch_predict(kind, device_forest(b), a, b.dev.num_cus, stream, tune));
    HIP_CHECK(launch_group_leaf_gather(b.d_gleaf.p, n, T, b.d_flat_of_file.p, L, d_out, stream));
    return;
  }
  const std::vector<uint32_t> cnt = group_tree_counts(b, L);
  b.d_planes.ensure((size_t)n * G);
  a.perm = cluster_rows(b, d, a, false, kind, stream);           // the rows' order: one pass for all groups
  // room for the leaves of the largest group's trees, made once: no buffer is replaced between the groups' launches
  if (a.perm == nullptr) leaf_room(b, n, *std::max_element(cnt.begin(), cnt.end()), tune, tune.grid_im, tune.grid_jm, tune.grid_row0);
  uint32_t base_bits = 0;
  memcpy(&base_bits, &b.margin_base, sizeof base_bits);
  for (uint32_t g = 0; g < G; ++g) {
    float* plane = b.d_planes.p + (size_t)g * n;
    if (cnt[g] == 0) {
      if (n) HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(plane), (int)base_bits, (size_t)n, stream));
      continue;
    }
    a.tree_begin = b.group_begin[g];
    a.tree_end = a.tree_begin + cnt[g];
    a.out = plane;
    LaunchTuning gt = tune;      // (not walk_with_buffers: the room above serves every group, the list is prepared per group)
    const bool deferring = a.perm == nullptr && d.ncol == 27 && defer_prepare(b, n, gt, stream);
    HIP_CHECK(launch_predict(kind, device_forest(b), a, b.dev.num_cus, stream, gt));
    if (deferring) defer_look(b, n, stream);
  }
  if (a.perm != nullptr) mark_cluster_in_flight(b, stream);
  HIP_CHECK(launch_group_finish(b.d_planes.p, n, G, finish, d_out, stream));
}

// The tables of an explanation call, and the refusals that come with them.  What a mode needs is built at
// its first call on the loaded model (contribs.hpp), on the booster's CURRENT device: the booster is uploaded first
// (ensure_uploaded: it may just have been moved by "ohx_device"), and device tables left on another device are
// released and built again here - so nothing a caller takes from the state or the booster afterwards (buffers,
// b.dev, b.s_exec) is stale.  A model that cannot have contributions keeps its reason and is refused again at once.
ContribsState& contribs_tables(BoosterObj& b, bool approximate, bool interactions = false) {
  if (!b.loaded) throw OhxError("the booster holds no model: call XGBoosterLoadModel first");
  if (!b.margin_error.empty()) throw OhxError(b.margin_error);
  if (!b.contribs) b.contribs.reset(new ContribsState());
  ContribsState& c = *b.contribs;
  if (!c.error.empty()) throw OhxError(c.error);
  if (!c.checked) {
    try {
      if (b.forest.num_feature > kMaxContribFeatures)
        throw OhxError("feature contributions support boosters of at most " + std::to_string(kMaxContribFeatures) +
                       " features (this one has " + std::to_string(b.forest.num_feature) + ")");
      check_contrib_cover(b.forest);
    } catch (const OhxError& e) {
      c.error = e.what();
      throw;
    }
    c.means.clear();
    for (const Tree& t : b.flat().trees) c.means.push_back(node_means(t));
    c.checked = true;
  }
  if (!approximate && !c.exact_error.empty()) throw OhxError(c.exact_error);
  PathTable pt;
  if (!approximate && !c.exact_ready) {      // host work first: a path that is too long is refused before any upload
    try {
      pt = build_path_table(b.flat());
    } catch (const OhxError& e) {
      c.exact_error = e.what();
      throw;
    }
  }
  ensure_uploaded(b);
  if (c.device != b.dev.ordinal) {
    if (c.device >= 0) {
      HIP_CHECK(hipSetDevice(c.device));
      c.release_device();
      HIP_CHECK(hipSetDevice(b.dev.ordinal));
      if (!approximate && pt.heads.empty() && !c.exact_ready) pt = build_path_table(b.flat());
    }
    c.device = b.dev.ordinal;
    c.d_flags.ensure(1);
    c.h_flags.ensure(1);
    HIP_CHECK(hipMemset(c.d_flags.p, 0, sizeof(uint32_t)));
  }
  if (!approximate && !c.exact_ready) {
    c.d_heads.upload(pt.heads);
    c.d_elems.upload(pt.elems);
    c.d_class_start.upload(pt.class_start);
    c.d_coef.upload(unwind_coefficients());
    c.exact_ready = true;
  }
  if (interactions && !approximate && !c.index_ready) {
    // the path table's host copy is not kept once it is on the device: build it again for the index
    if (pt.heads.empty()) pt = build_path_table(b.flat());
    const FeaturePathIndex ix = build_feature_path_index(pt, (uint32_t)b.flat().trees.size(), b.forest.num_feature);
    c.d_fpaths.upload(ix.paths);
    c.d_fstart.upload(ix.start);
    c.index_ready = true;
  }
  if (approximate && !c.approx_ready) {
    std::vector<uint32_t> roots;
    c.d_nodes.upload(emit_contrib_nodes(b.flat(), c.means, &roots));
    c.d_roots.upload(roots);
    c.approx_ready = true;
  }
  return c;
}

// (shared with the selected-gridcells calls, which take no booster)
void check_grid_positive(int im, int jm, int km) {
  if (im <= 0 || jm <= 0 || km <= 0) throw OhxError("predict_fields: im, jm, km must be positive");
}

// the fields forms' checks of the grid and the field count (predict and contributions)
void check_fields_shape(const BoosterObj& b, int nfield, int im, int jm, int km, int k1, int k2) {
  if (nfield < 0 || nfield > 32) throw OhxError("predict_fields: nfield must be 0..32");
  if ((uint32_t)nfield > b.forest.num_feature)
    throw OhxError("Number of columns does not match number of features in booster (" + std::to_string(nfield) +
                   " vs. " + std::to_string(b.forest.num_feature) + ")");
  if (b.forest.num_feature > 32) throw OhxError("predict_fields supports boosters with at most 32 features");
  check_grid_positive(im, jm, km);
  if (k1 < 1 || k2 > km || k2 < k1 - 1) throw OhxError("predict_fields: need 1 <= k1, k2 <= km, k2 >= k1 - 1");
}

// The fields forms' preamble, into any of their argument structs (FieldsArgs, FieldsContribsArgs, GatherCellsArgs): which
// fields are (im,jm), the feature divided by 100 or none, the field count - and no field NULL (`fields` null: the caller
// looks at its fields itself, as it stages them).
template <class Args>
void fields_preamble(Args& a, const float* const fields[], const int32_t is2d[], int nfield, int pl_feature) {
  a.is2d_mask = 0;
  for (int f = 0; f < nfield; ++f) {
    if (fields != nullptr && fields[f] == nullptr) throw OhxError("predict_fields: field " + std::to_string(f) + " is NULL");
    if (is2d[f]) a.is2d_mask |= 1u << f;
  }
  a.pl_feature = pl_feature < 0 ? 0xFFFFFFFFu : (uint32_t)pl_feature;
  a.nfield = (uint32_t)nfield;
}

// ---- explanations: feature contributions and SHAP interaction values (docs/12_contributions.md, "The call path") ----
//
// One path for all eight ABI functions, each step once: explain_refusals, explain_args / interactions_args, then in
// explain() the room, the enqueue and, for a host form, finish_host_form.  Every refusal and every allocation comes
// before anything is enqueued.

// the fields forms' arguments, as the ABI takes them (host or device pointers, by the form)
struct FieldsSource {
  const float* const* fields;
  const int32_t* is2d;
  int nfield, pl_feature, im, jm, km, k1, k2;
  float missing;
  float* const* out;               // [F + 1], NULL = not stored
};

// What one call asks for.  The source is a DMatrix (rows forms) or the fields arguments (fields forms).
struct ExplainCall {
  const char* name = "";           // the ABI function, for the messages
  bool interactions = false;       // SHAP interaction values, else feature contributions
  int approximate = 0;             // as given: refused unless 0 or 1
  unsigned ntree_limit = 0;
  bool host_form = false;          // on the library's stream, through the state's buffers; else enqueued on `stream`
  hipStream_t stream = nullptr;
  DMatrixObj* d = nullptr;         // rows forms
  float* d_out = nullptr;          // rows forms, device form
  const FieldsSource* fs = nullptr;
};
struct ExplainResult {
  size_t count = 0;                // floats of a rows form's output
  float* host = nullptr;           // the host form's copy of it
};

// Every refusal, in the order the forms have always had, building on the way what the mode needs (contribs_tables:
// after it the booster is settled on its device, so its stream and the state's buffers may be taken).  A fields form's
// preamble goes to `fa`.
ContribsState& explain_refusals(BoosterObj& b, const ExplainCall& q, FieldsContribsArgs& fa) {
  const FieldsSource* fs = q.fs;
  if (fs != nullptr && (fs->fields == nullptr || fs->is2d == nullptr || fs->out == nullptr))
    throw OhxError("predict_fields: NULL argument");
  if (q.approximate != 0 && q.approximate != 1) throw OhxError("approximate must be 0 (exact TreeSHAP) or 1");
  if (!b.loaded) throw OhxError("the booster holds no model: call XGBoosterLoadModel first");
  if (fs == nullptr && !q.host_form && q.d_out == nullptr && q.d->nrow != 0)
    throw OhxError(std::string(q.name) + ": d_out is NULL");
  // before the tables are built: building them waits for the library's stream
  if (!q.host_form && stream_capturing(q.stream))
    refuse_in_capture(q.interactions ? "compute SHAP interaction values" : "compute feature contributions",
                      (std::string(q.name) + " is not capturable; call it outside the capture").c_str());
  if (fs != nullptr) {
    check_fields_shape(b, fs->nfield, fs->im, fs->jm, fs->km, fs->k1, fs->k2);
    fields_preamble(fa, fs->fields, fs->is2d, fs->nfield, fs->pl_feature);
    bool any_out = false;
    for (uint32_t f = 0; f <= b.forest.num_feature; ++f) any_out |= fs->out[f] != nullptr;
    if (!any_out) throw OhxError("feature contributions from fields: every entry of out is NULL");
  } else {
    check_columns(b, q.d->ncol);
  }
  ContribsState& c = contribs_tables(b, q.approximate != 0, q.interactions);
  if (fs != nullptr) return c;
  const DMatrixObj& d = *q.d;
  check_same_device(d, b.dev.ordinal);
  if (q.interactions) {
    const uint64_t F1 = (uint64_t)b.forest.num_feature + 1, W = F1 * F1, G = b.num_groups;
    if (d.nrow > (uint64_t)(SIZE_MAX / sizeof(float)) / (W * G))
      throw OhxError("SHAP interaction values: " + std::to_string(d.nrow) + " rows of " +
                     (G >= 2 ? std::to_string(G) + " x " : std::string()) + std::to_string(W) +
                     " floats do not fit in memory");
  }
  return c;
}

// The one place a ContribsArgs gets its trees, its bias and the mode's tables; the caller adds the rows and the output.
ContribsArgs explain_args(const BoosterObj& b, const ContribsState& c, uint32_t t0, uint32_t t1) {
  ContribsArgs a;
  a.nfeat = b.forest.num_feature;
  a.tree_begin = t0;
  a.tree_end = t1;
  a.bias = contrib_bias(b.flat(), c.means, t0, t1, b.margin_base);
  a.heads = c.d_heads.p;
  a.elems = c.d_elems.p;
  a.class_start = c.d_class_start.p;
  a.coef = c.d_coef.p;
  a.nodes = c.d_nodes.p;
  a.roots = c.d_roots.p;
  return a;
}

// ... and an InteractionsArgs: the rows and trees of `a`, whose output is the phi this one reads.
InteractionsArgs interactions_args(const ContribsArgs& a, const ContribsState& c, float* out) {
  InteractionsArgs ia;
  ia.rows = a.rows;
  ia.nrow = a.nrow;
  ia.ncol = a.ncol;
  ia.missing = a.missing;
  ia.nfeat = a.nfeat;
  ia.tree_begin = a.tree_begin;
  ia.tree_end = a.tree_end;
  ia.phi = a.out;
  ia.out = out;
  ia.heads = c.d_heads.p;
  ia.elems = c.d_elems.p;
  ia.fpaths = c.d_fpaths.p;
  ia.fstart = c.d_fstart.p;
  ia.coef = c.d_coef.p;
  return ia;
}

// The end of a host form: the output (or each requested output's slab) and the inf flag come back, and a set flag is
// cleared for the next call and refused.
struct CopyBack {
  float* dst;
  const float* src;
  size_t count;
};
void finish_host_form(ContribsState& c, hipStream_t s, const std::vector<CopyBack>& copies) {
  for (const CopyBack& k : copies)
    if (k.count) HIP_CHECK(hipMemcpyAsync(k.dst, k.src, k.count * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(c.h_flags.p, c.d_flags.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (c.h_flags.p[0] != 0) {
    HIP_CHECK(hipMemsetAsync(c.d_flags.p, 0, sizeof(uint32_t), s));
    HIP_CHECK(hipStreamSynchronize(s));
    throw OhxError("Input data contains `inf` or `nan`");
  }
}

// The call.  A single-group booster is one tree range written straight to the output; several output groups are one
// range each - [nrow][G][W], W = F+1 or (F+1)^2 - computed into the state's block buffer and scattered from there to
// the group's place.  Contributions keep d_out / h_out / d_part and interactions d_iout / h_iout / d_ipart: a result
// stays valid until the next call of its own kind (include/ohxgb.h).  Returns what a rows host form hands back; the
// state is dropped by nothing before the next explanation call on the booster.
ExplainResult explain(BoosterObj& b, const ExplainCall& q) {
  FieldsContribsArgs fa;
  ContribsState& c = explain_refusals(b, q, fa);
  const FieldsSource* fs = q.fs;
  if (fs != nullptr && fs->k2 < fs->k1) return {};
  const bool approx = q.approximate != 0;
  const uint32_t F = b.forest.num_feature, G = b.num_groups;
  const uint64_t F1 = (uint64_t)F + 1, W = q.interactions ? F1 * F1 : F1;
  const uint64_t plane = fs ? (uint64_t)fs->im * (uint64_t)fs->jm : 0;
  const uint64_t nrow = fs ? plane * (uint64_t)(fs->k2 - fs->k1 + 1) : q.d->nrow;
  const uint64_t slab = fs ? plane * (uint64_t)(fs->k1 - 1) : 0;     // floats from a 3-D array's start to level k1

  // the tree ranges and their launch shapes
  struct Range {
    uint32_t t0, t1;
    ContribsPlan cplan, iplan;
  };
  std::vector<Range> ranges(G >= 2 ? G : 1);
  if (G >= 2) {
    const std::vector<uint32_t> cnt = group_tree_counts(b, group_tree_limit(b, q.ntree_limit));
    for (uint32_t g = 0; g < G; ++g) {
      ranges[g].t0 = b.group_begin[g];
      ranges[g].t1 = ranges[g].t0 + cnt[g];
    }
  } else {
    tree_range(b, q.ntree_limit, &ranges[0].t0, &ranges[0].t1);
  }
  uint64_t part = 0;
  for (Range& r : ranges) {
    r.cplan = plan_contribs(nrow, F, r.t1 - r.t0, b.contribs_split);
    if (q.interactions && !approx) r.iplan = plan_interactions(nrow, F, r.t1 - r.t0, b.contribs_split);
    part = std::max({part, r.cplan.part_floats, r.iplan.part_floats});
  }

  // room: every buffer of the call, before the first enqueue
  DevBuf<float>& d_part = q.interactions ? c.d_ipart : c.d_part;
  ExplainResult res;
  float* out = q.d_out;
  if (fs != nullptr) {
    if (q.host_form) {
      uint32_t nout = 0;
      for (uint32_t f = 0; f <= F; ++f) nout += fs->out[f] != nullptr ? 1u : 0u;
      if (c.d_fstage.size() < (size_t)fs->nfield) c.d_fstage.resize((size_t)fs->nfield);
      for (int f = 0; f < fs->nfield; ++f) c.d_fstage[(size_t)f].ensure(fs->is2d[f] ? plane : nrow);
      c.d_fout.ensure((size_t)(nout * nrow));
    }
  } else {
    res.count = (size_t)(nrow * G * W);
    if (q.host_form) {
      DevBuf<float>& d_res = q.interactions ? c.d_iout : c.d_out;
      PinnedBuf<float>& h_res = q.interactions ? c.h_iout : c.h_out;
      d_res.ensure(res.count);
      h_res.ensure(res.count);
      out = d_res.p;
      res.host = h_res.p;
    }
    if (q.interactions) c.d_iphi.ensure((size_t)(nrow * F1));
    if (G >= 2) c.d_gblock.ensure((size_t)(nrow * W));
  }
  if (part) d_part.ensure((size_t)part);

  // enqueue: a host form on the library's stream of the booster's device, behind what the caller's default stream
  // holds for a matrix that borrows the caller's rows
  hipStream_t stream = q.host_form ? b.s_exec : q.stream;
  std::vector<CopyBack> back;
  if (fs != nullptr) {
    fa.missing = fs->missing;
    fa.plane = plane;
    fa.nrow = nrow;
    if (q.host_form) {
      // 3-D fields: the slab's levels only, as the fields predict stages them
      for (int f = 0; f < fs->nfield; ++f) {
        float* dst = c.d_fstage[(size_t)f].p;
        const bool flat = fs->is2d[f] != 0;
        HIP_CHECK(hipMemcpyAsync(dst, fs->fields[f] + (flat ? 0 : slab), (flat ? plane : nrow) * sizeof(float),
                                 hipMemcpyHostToDevice, stream));
        fa.field[f] = dst;
      }
      for (uint32_t f = 0; f <= F; ++f) {
        if (fs->out[f] == nullptr) continue;
        fa.out[f] = c.d_fout.p + back.size() * (size_t)nrow;
        back.push_back({fs->out[f] + slab, fa.out[f], (size_t)nrow});
      }
      fa.flags = c.d_flags.p;
    } else {
      for (int f = 0; f < fs->nfield; ++f) fa.field[f] = fs->fields[f];
      for (uint32_t f = 0; f <= F; ++f) fa.out[f] = fs->out[f];
      fa.src_off = fa.out_off = slab;
    }
  } else if (q.host_form) {
    if (q.d->owned == nullptr) order_behind_caller(b.dev.ordinal, stream);
    back.push_back({res.host, out, res.count});
  }
  for (uint32_t g = 0; g < (uint32_t)ranges.size(); ++g) {
    const Range& r = ranges[g];
    ContribsArgs a = explain_args(b, c, r.t0, r.t1);
    float* target = G >= 2 ? c.d_gblock.p : out;
    if (fs != nullptr) {
      a.missing = fs->missing;
      HIP_CHECK((hipError_t)launch_contribs_fields(approx, a, fa, r.cplan, d_part.p, stream));
      continue;
    }
    a.rows = q.d->d_data;
    a.nrow = nrow;
    a.ncol = (uint32_t)q.d->ncol;
    a.missing = q.d->missing;
    if (q.host_form) a.flags = c.d_flags.p;
    a.out = q.interactions ? c.d_iphi.p : target;
    HIP_CHECK((hipError_t)launch_contribs(approx, a, r.cplan, d_part.p, stream));
    if (q.interactions)   // the matrix, behind the phi it reads on the same stream
      HIP_CHECK((hipError_t)launch_interactions(approx, interactions_args(a, c, target), r.iplan, d_part.p, stream));
    if (G >= 2) HIP_CHECK(launch_group_block_scatter(c.d_gblock.p, nrow, (uint32_t)W, G, g, out, stream));
  }
  if (q.host_form) finish_host_form(c, stream, back);
  return res;
}

// ---- the leaf walk the visit counts and the refit share ----

// the host part, built at first use on the loaded model; no device needed
LeafWalkState& leaf_walk_host(BoosterObj& b) {
  if (!b.leaf_walk) {
    auto w = std::make_unique<LeafWalkState>();
    w->vf = emit_visits(b.forest, place_forest(b.forest, b.layout));
    b.leaf_walk = std::move(w);
  }
  return *b.leaf_walk;
}

// The booster's device (where it has one already), without building any of the predict path's device forms; throws
// where there is no usable HIP device.
DeviceInfo leaf_walk_device(const BoosterObj& b) { return use_device(b.uploaded ? b.dev.ordinal : b.device_pref); }

// Builds the walk on `dev` (leaf_walk_device); one left on another device is freed first, so that no buffer stays
// behind there.  Waits for the library's stream: never called inside a capture.
LeafWalkState& leaf_walk_on_device(BoosterObj& b, const DeviceInfo& dev) {
  LeafWalkState& w = leaf_walk_host(b);
  if (w.device != dev.ordinal) {
    w.d_nodes.release();
    w.d_roots.release();
    w.d_leaf_offset.release();
    w.d_nodes.upload(w.vf.nodes);
    w.d_roots.upload(w.vf.roots);
    w.d_leaf_offset.upload(w.vf.leaf_offset);
    w.device = dev.ordinal;
    w.num_cus = dev.num_cus;
  }
  return w;
}

DeviceLeafWalk device_leaf_walk(const BoosterObj& b, const LeafWalkState& w) {
  // nodes, node_bytes, roots, leaf_offset, num_trees, num_feature, total_leaves
  return {w.d_nodes.p, (uint32_t)(w.vf.nodes.size() * sizeof(VisitNode)), w.d_roots.p, w.d_leaf_offset.p,
          (uint32_t)b.forest.trees.size(), b.forest.num_feature, w.vf.leaf_offset.back()};
}

// ---- node visit counts (visits.hpp) ----

// What every one of the five calls refuses first, then the host parts (built at first use; no device needed)
VisitState& visits_begin(BoosterObj& b, const char* what) {
  if (!b.loaded) throw OhxError("the booster holds no model: call XGBoosterLoadModel first");
  refuse_categorical(b, what);
  refuse_groups(b, what);
  const LeafWalkState& w = leaf_walk_host(b);
  if (!b.visits) {
    b.visits = std::make_unique<VisitState>();
    b.visits->node_counts.assign((size_t)w.vf.tree_offsets.back(), 0);
  }
  return *b.visits;
}

// The device part, and the plan's tree lists for the knobs as they stand.  Waits for the library's stream: never called
// inside a capture.
LeafWalkState& visits_on_device(BoosterObj& b, VisitState& v) {
  LeafWalkState& w = leaf_walk_on_device(b, leaf_walk_device(b));
  if (v.device != w.device) {
    hipStream_t exec = lib_streams(w.device).exec;
    const size_t leaves = w.vf.leaf_offset.back();
    v.d_counts.release();                                // (counters left on another device go with it)
    for (DevBuf<uint32_t>* buf : {&v.d_lds_trees, &v.d_global_trees}) buf->release();
    v.d_counts.ensure(std::max<size_t>(leaves, 1));      // (a forest without trees: the memset below writes one word)
    v.h_leaf.ensure(std::max<size_t>(leaves, 1));
    HIP_CHECK(hipMemsetAsync(v.d_counts.p, 0, std::max<size_t>(leaves, 1) * sizeof(unsigned long long), exec));
    HIP_CHECK(hipStreamSynchronize(exec));
    v.rows_seen = 0;
    v.plan_uploaded = false;
    v.device = w.device;
  }
  if (!v.plan_uploaded || v.plan_lds_leaves != b.visits_lds_leaves || v.plan_use_lds != b.visits_use_lds) {
    // (a count enqueued earlier may still read the lists: the upload below waits for the library's stream only)
    if (v.plan_uploaded) HIP_CHECK(hipDeviceSynchronize());
    v.plan = plan_visits(w.vf, b.forest.num_feature, b.visits_lds_leaves, /*force_global=*/!b.visits_use_lds);
    v.d_lds_trees.upload(v.plan.lds_trees);
    v.d_global_trees.upload(v.plan.global_trees);
    HIP_CHECK((hipError_t)prepare_count_visits(v.plan));      // once per plan: the kernels' dynamic LDS limits
    v.plan_lds_leaves = b.visits_lds_leaves;
    v.plan_use_lds = b.visits_use_lds;
    v.plan_uploaded = true;
  }
  return w;
}

// The booster's refusals come before the matrix handle is looked at.
void count_visits(BoosterObj& b, DMatrixHandle dmat, bool host_form, hipStream_t caller, const char* what) {
  VisitState& v = visits_begin(b, what);
  DMatrixObj& d = *as_dmat(dmat);
  check_columns(b, d.ncol);
  // before the device part is built: building it waits for the library's stream
  if (!host_form && stream_capturing(caller))
    refuse_in_capture("count node visits", (std::string(what) + " is not capturable; call it outside the capture").c_str());
  const LeafWalkState& w = visits_on_device(b, v);
  check_same_device(d, w.device);
  hipStream_t stream = host_form ? lib_streams(w.device).exec : caller;
  if (host_form && d.owned == nullptr) order_behind_caller(w.device, stream);
  DeviceVisitForest fr;
  fr.walk = device_leaf_walk(b, w);
  fr.lds_trees = v.d_lds_trees.p;
  fr.global_trees = v.d_global_trees.p;
  VisitArgs a;
  a.rows = d.d_data;
  a.nrow = d.nrow;
  a.ncol = (uint32_t)d.ncol;
  a.missing = d.missing;
  a.counts = v.d_counts.p;
  HIP_CHECK((hipError_t)launch_count_visits(fr, a, v.plan, w.num_cus, tune_for(b, d), stream));
  v.rows_seen += d.nrow;
  if (host_form) HIP_CHECK(hipStreamSynchronize(stream));
  else d.used_async = true;
}

// Waits for `stream`, brings the leaf counters back and sums them up each tree (v.node_counts).  A state that has never
// counted has no device part: all zeros.
void read_visit_counts(BoosterObj& b, VisitState& v, hipStream_t stream) {
  const LeafWalkState& w = leaf_walk_host(b);
  const size_t leaves = w.vf.leaf_offset.back();
  if (v.device < 0) {
    std::fill(v.node_counts.begin(), v.node_counts.end(), 0);
    return;
  }
  HIP_CHECK(hipSetDevice(v.device));
  if (leaves) HIP_CHECK(hipMemcpyAsync(v.h_leaf.p, v.d_counts.p, leaves * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are uint64");
  visit_node_sums(b.forest, w.vf, reinterpret_cast<const uint64_t*>(v.h_leaf.p), v.node_counts.data());
}

// "ohx_monotone_constraints": `(` entries `)` separated by `,`, each -1, 0, 1 or +1, spaces and tabs between tokens; at most
// kGrowMaxConstraints entries.  A list of zeros is the default and comes back empty.
std::vector<int8_t> parse_monotone_constraints(const char* value) {
  const OhxError bad("ohx_monotone_constraints must be a list such as (1,0,-1): entries -1, 0, 1 or +1 in parentheses, separated by "
                     "commas, at most 128 of them");
  std::vector<int8_t> c;
  const char* p = value;
  auto blanks = [&]() {
    while (*p == ' ' || *p == '\t') ++p;
  };
  blanks();
  if (*p++ != '(') throw bad;
  blanks();
  if (*p != ')') {
    for (;;) {
      int8_t v;
      if (p[0] == '0') v = 0, p += 1;
      else if (p[0] == '1') v = 1, p += 1;
      else if (p[0] == '+' && p[1] == '1') v = 1, p += 2;
      else if (p[0] == '-' && p[1] == '1') v = -1, p += 2;
      else throw bad;
      if (c.size() == kGrowMaxConstraints) throw bad;
      c.push_back(v);
      blanks();
      if (*p == ')') break;
      if (*p++ != ',') throw bad;
      blanks();
    }
  }
  ++p;
  blanks();
  if (*p != '\0') throw bad;
  if (std::all_of(c.begin(), c.end(), [](int8_t v) { return v == 0; })) c.clear();
  return c;
}

// "ohx_interaction_constraints": grow.cpp's grow_interact_parse; a refused value throws and leaves the caller's as it was.
std::vector<uint64_t> parse_interaction_constraints(const char* value) {
  std::vector<uint64_t> groups;
  if (!grow_interact_parse(value, &groups))
    throw OhxError("ohx_interaction_constraints must be a list of groups such as [[0,2],[1,3,4]]: at most 64 groups in brackets, "
                   "separated by commas, each a non-empty list of distinct feature ids below 128 in brackets; [] sets none");
  return groups;
}

// ---- leaf refit (refit.hpp) ----

// Both forms of OHXBoosterRefitLeaves.  The refusals that need neither a matrix nor a device come first, in the
// header's order; nothing is enqueued before the last of them.
void refit_leaves(BoosterObj& b, DMatrixHandle dmat, const float* labels, bst_ulong nlabel, float eta, float lambda,
                  int unvisited, bst_ulong* leaves_refit, bool host_form, hipStream_t caller, const char* what) {
  if (!b.loaded) throw OhxError("the booster holds no model: call XGBoosterLoadModel first");
  refuse_categorical(b, what);
  refuse_groups(b, what);
  if (!objective_is_identity(b.forest.objective))
    throw OhxError(std::string(what) + " refits squared-error leaves (gradient pred - label, hessian 1): the objective " +
                   b.forest.objective + " is not reg:squarederror");
  if (b.grow_objective != kGrowObjSquared)
    throw OhxError(std::string(what) + " refits squared-error leaves (hessian 1 a row): it is refused while ohx_objective=" +
                   grow_objective_name(b.grow_objective) + " "
                   "is set; grow with OHXBoosterBoostTreesWeighted, or set ohx_objective=squarederror; nothing was enqueued");
  if (b.grow_alpha != 0.0f || b.grow_max_delta_step != 0.0f)
    throw OhxError(std::string(what) + " refits unregularised leaves: it is refused while ohx_reg_alpha or ohx_max_delta_step is set; "
                   "grow with OHXBoosterBoostTreesWeighted, or set both to 0; nothing was enqueued");
  if (!b.grow_mono.empty())
    throw OhxError(std::string(what) + " refits every leaf on its own and would undo the weight intervals: it is refused while "
                   "ohx_monotone_constraints is active; grow with OHXBoosterBoostTreesWeighted, or set it to (); nothing was enqueued");
  if (labels == nullptr) throw OhxError(std::string(what) + ": labels is NULL");
  if (!std::isfinite(eta)) throw OhxError(std::string(what) + ": eta must be finite");
  if (!(std::isfinite(lambda) && lambda >= 0.0f)) throw OhxError(std::string(what) + ": lambda must be finite and >= 0");
  if (unvisited != 0 && unvisited != 1) throw OhxError(std::string(what) + ": unvisited must be 0 (keep) or 1 (zero)");
  DMatrixObj& d = *as_dmat(dmat);
  if (d.nrow == 0) throw OhxError(std::string(what) + ": the matrix has no rows");
  if (nlabel != d.nrow)
    throw OhxError(std::string(what) + ": " + std::to_string(nlabel) + " labels for " + std::to_string(d.nrow) + " rows");
  if (d.nrow > kRefitMaxRows)
    throw OhxError(std::string(what) + ": at most 2^31 rows per refit (" + std::to_string(d.nrow) + " given)");
  check_columns(b, d.ncol);
  // before anything is built or enqueued: building the state waits for the library's stream
  if (!host_form && stream_capturing(caller))
    refuse_in_capture("refit leaf values", (std::string(what) + " is not capturable; call it outside the capture").c_str());
  const DeviceInfo dev = leaf_walk_device(b);   // throws where there is no device
  check_same_device(d, dev.ordinal);
  if (!b.refit) b.refit = std::make_unique<RefitState>();
  RefitState& r = *b.refit;
  const LeafWalkState& w = leaf_walk_on_device(b, dev);
  const size_t T = b.forest.trees.size();
  const size_t leaves = w.vf.leaf_offset.back();
  const RefitPlan plan = plan_refit(d.nrow, b.forest.num_feature, T, dev.num_cus);
  if (r.device != w.device) {
    for (DevBuf<uint32_t>* buf : {&r.d_ids, &r.d_error}) buf->release();      // (what was left on another device)
    for (DevBuf<float>* buf : {&r.d_pred, &r.d_leaf, &r.d_weight, &r.d_labels}) buf->release();
    for (DevBuf<unsigned long long>* buf : {&r.d_G, &r.d_H}) buf->release();
    // (a forest without trees has no leaf: one word each, so that the memsets below have somewhere to go)
    const size_t room = std::max<size_t>(leaves, 1);
    r.d_G.ensure(room);
    r.d_H.ensure(room);
    r.d_leaf.ensure(room);
    r.d_weight.ensure(room);
    r.d_error.ensure(1);
    r.h_leaf.ensure(room);
    r.h_weight.ensure(room);
    r.h_H.ensure(room);
    r.h_error.ensure(1);
    r.device = w.device;
    r.prepared = false;
  }
  if (!r.prepared) {
    HIP_CHECK((hipError_t)prepare_refit(plan));
    r.prepared = true;
  }
  try {
    r.d_ids.ensure((size_t)T * d.nrow);
  } catch (const OhxError& e) {
    throw OhxError(std::string(what) + ": the leaf-id buffer of " + std::to_string(T) + " trees x " + std::to_string(d.nrow) +
                   " rows x 4 = " + std::to_string(plan.ids_bytes) + " bytes cannot be allocated (" + e.what() + ")");
  }
  r.d_pred.ensure(d.nrow);
  if (host_form) r.d_labels.ensure(d.nrow);
  hipStream_t stream = host_form ? lib_streams(dev.ordinal).exec : caller;
  if (host_form && d.owned == nullptr) order_behind_caller(dev.ordinal, stream);
  // every earlier refit has been waited for, so the buffers are free; the old leaf tables go in, for the leaves no row
  // reaches
  refit_gather_leaves(b.forest, w.vf, r.h_leaf.p, r.h_weight.p);
  const size_t nl = std::max<size_t>(leaves, 1);
  HIP_CHECK(hipMemsetAsync(r.d_G.p, 0, nl * sizeof(unsigned long long), stream));
  HIP_CHECK(hipMemsetAsync(r.d_H.p, 0, nl * sizeof(unsigned long long), stream));
  HIP_CHECK(hipMemsetAsync(r.d_error.p, 0, sizeof(uint32_t), stream));
  if (leaves) {
    HIP_CHECK(hipMemcpyAsync(r.d_leaf.p, r.h_leaf.p, leaves * sizeof(float), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(r.d_weight.p, r.h_weight.p, leaves * sizeof(float), hipMemcpyHostToDevice, stream));
  }
  if (host_form) HIP_CHECK(hipMemcpyAsync(r.d_labels.p, labels, d.nrow * sizeof(float), hipMemcpyHostToDevice, stream));
  RefitArgs a;
  a.walk = device_leaf_walk(b, w);
  a.rows = d.d_data;
  a.nrow = d.nrow;
  a.ncol = (uint32_t)d.ncol;
  a.missing = d.missing;
  a.labels = host_form ? r.d_labels.p : labels;
  a.ids = r.d_ids.p;
  a.pred = r.d_pred.p;
  a.G = r.d_G.p;
  a.H = r.d_H.p;
  a.leaf = r.d_leaf.p;
  a.weight = r.d_weight.p;
  a.error = r.d_error.p;
  a.base = b.margin_base;
  a.eta = eta;
  a.lambda = lambda;
  a.unvisited = unvisited;
  hipError_t launched = (hipError_t)launch_refit(a, plan, w.vf.leaf_offset.data(), stream);
  if (launched == hipSuccess && leaves) {
    launched = hipMemcpyAsync(r.h_leaf.p, r.d_leaf.p, leaves * sizeof(float), hipMemcpyDeviceToHost, stream);
    if (launched == hipSuccess) launched = hipMemcpyAsync(r.h_weight.p, r.d_weight.p, leaves * sizeof(float), hipMemcpyDeviceToHost, stream);
    if (launched == hipSuccess) launched = hipMemcpyAsync(r.h_H.p, r.d_H.p, leaves * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream);
  }
  if (launched == hipSuccess) launched = hipMemcpyAsync(r.h_error.p, r.d_error.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
  // both forms wait, whatever was enqueued: the labels and the tables are read from the caller's and the state's memory
  const hipError_t waited = hipStreamSynchronize(stream);
  if (!host_form) d.used_async = true;
  HIP_CHECK(launched);
  HIP_CHECK(waited);
  const uint32_t flags = r.h_error.p[0];
  if (flags & kRefitFlagLabel)
    throw OhxError(std::string(what) + ": a gradient pred - label is not finite or reaches 256 in size at some row and tree: "
                   "look for a label that is NaN, infinite or far from the model's range; the forest is unchanged");
  if (flags != 0) throw OhxError(std::string(what) + ": the refit kernels reported error flags " + std::to_string(flags));
  // all or nothing: every tree is done and the error word is clean
  refit_write_back(b.forest, w.vf, r.h_leaf.p, r.h_weight.p);
  // everything built from leaf values is dropped as a model load drops it; the visit state holds none
  invalidate_device_state(b);
  b.contribs.reset();
  if (leaves_refit != nullptr) {
    bst_ulong n = 0;
    for (size_t l = 0; l < leaves; ++l) n += r.h_H.p[l] != 0ull ? 1u : 0u;
    *leaves_refit = n;
  }
}

// ---- boosting new trees (grow.hpp) ----

// The optional parts of a boost call.  OHXBoosterBoostTreesEval adds the held-out set, the patience and where the
// results go; OHXBoosterBoostTreesWeighted the weights of both sets (either may be NULL: all 1.0f) and min_child_weight
// in place of min_child_rows; OHXBoosterBoostTreesSampled the fraction of the rows and of the features a tree sees, and
// the seed of the draws.
struct BoostEval {
  bool present = false;
  DMatrixHandle dmat = nullptr;      // NULL: no held-out set
  const float* labels = nullptr;
  bst_ulong nlabel = 0;
  int patience = 0;
  double* train_rmse = nullptr;
  double* eval_rmse = nullptr;
  int* rounds_run = nullptr;
  int* best_round = nullptr;
};
struct BoostWeights {
  bool present = false;
  const float* weights = nullptr;
  const float* eval_weights = nullptr;
  float min_child_weight = 0.0f;
};
struct BoostSampling {
  bool present = false;
  float subsample = 1.0f;
  float colsample_bytree = 1.0f;
  uint64_t seed = 0;
};

// One call of any OHXBoosterBoostTrees* entry point: the training set, the hyper-parameters, the optional parts, and
// the form (host arrays staged on the library's stream, or device arrays on the caller's).
struct BoostCall {
  const char* what = "";
  bool host_form = true;
  hipStream_t caller = nullptr;
  DMatrixHandle dmat = nullptr;
  const float* labels = nullptr;
  bst_ulong nlabel = 0;
  const bst_ulong* cut_ptr = nullptr;
  const float* cut_values = nullptr;
  int rounds = 0, max_depth = 0;
  float eta = 0.0f, lambda = 0.0f, gamma = 0.0f;
  bst_ulong min_child_rows = 1;      // not looked at where `weights` is present
  bst_ulong* nodes_added = nullptr;
  BoostEval eval;
  BoostWeights weights;
  BoostSampling sampling;
  bool deep = false;                 // OHXBoosterBoostTreesDeep and ...DeepSampled: max_depth up to 18
};

BoostCall boost_call(const char* what, bool host_form, void* stream, DMatrixHandle dmat, const float* labels, bst_ulong nlabel,
                     const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth, float eta, float lambda,
                     float gamma, bst_ulong* nodes_added) {
  BoostCall c;
  c.what = what;
  c.host_form = host_form;
  c.caller = static_cast<hipStream_t>(stream);
  c.dmat = dmat;
  c.labels = labels;
  c.nlabel = nlabel;
  c.cut_ptr = cut_ptr;
  c.cut_values = cut_values;
  c.rounds = rounds;
  c.max_depth = max_depth;
  c.eta = eta;
  c.lambda = lambda;
  c.gamma = gamma;
  c.nodes_added = nodes_added;
  return c;
}

BoostEval boost_eval(DMatrixHandle dmat, const float* labels, bst_ulong nlabel, int patience, double* train_rmse,
                     double* eval_rmse, int* rounds_run, int* best_round) {
  BoostEval ev;
  ev.present = true;
  ev.dmat = dmat;
  ev.labels = labels;
  ev.nlabel = nlabel;
  ev.patience = patience;
  ev.train_rmse = train_rmse;
  ev.eval_rmse = eval_rmse;
  ev.rounds_run = rounds_run;
  ev.best_round = best_round;
  return ev;
}

BoostWeights boost_weights(const float* weights, const float* eval_weights, float min_child_weight) {
  BoostWeights wt;
  wt.present = true;
  wt.weights = weights;
  wt.eval_weights = eval_weights;
  wt.min_child_weight = min_child_weight;
  return wt;
}

// The kind of a call, and in one place what it runs: its level plan, its tree launcher, its metric launchers and the
// layout of its metric sums (the words of one sum, where sum (t, set) lies, and the words in all for `rounds` rounds).
// Plain: row counts and 12-byte bins.  Weighted: fixed-point hessians.  Sampled: the same over a bag and a feature list.
// Deep: the weighted kind to level 7 and histograms in HBM from level 8 on, with its own node stride and held-out walk;
// `deep` is its plan and `deep_args` what its kernels take beyond GrowArgs (filled by boost_trees once the buffers stand).
// It answers with or without sampling: over a bag and a feature list its levels to 7 are the sampled kind's, and its plan
// is the one over the tree's columns.
// (Calls, not a table of function addresses: a build of this file alone links without the grower until it is used.)
struct BoostKind {
  enum Which { Plain, Weighted, Sampled, Deep } which;
  GrowDeepPlan deep;
  GrowDeepArgs deep_args;
  GrowLevelState* h_state = nullptr;   // where the Deep kind's tree launcher waits for the level word
  // pairs or inline: with `pairs` a round's (gradient, hessian) pairs are made once by grow_pairs.hip's pair kernel and
  // its histogram kernels read them (every objective but squared error, and squared error under ohx_grow_pairs = on);
  // without, the histogram kernels of the kind make g = pred - label themselves
  bool pairs = false;
  GrowPairArgs pair_args;
  // regularised (ohx_reg_alpha or ohx_max_delta_step is not 0; then `pairs` holds too): the pair path with grow_reg.hip's
  // split launches.  metric: what a row adds to the sums; away from rmse the metric kernels are grow_reg.hip's.  The two
  // choices are independent, and with neither nothing of grow_reg.hip is touched.
  // constrained (ohx_monotone_constraints holds an entry that is not 0; then `pairs` holds too, and `regularised` is not
  // asked): the pair path with grow_mono.hip's split launches, which carry alpha and max_delta_step themselves.  Without
  // it nothing of grow_mono.hip is touched.
  // column-sampled (ohx_colsample_bylevel or ohx_colsample_bynode takes a feature away from a level or a node; then
  // `pairs` holds too): the pair path over the level's list with grow_colsample.hip's split launches, under the policy
  // `regularised` / `constrained` name or the fixed-point one.  Without it nothing of grow_colsample.hip is touched.
  // interacting (ohx_interaction_constraints takes a candidate away from some node; then `pairs` holds too, and
  // `colsampled` and `quantile` do not): the pair path with grow_interact.hip's split launches, under the policy
  // `regularised` / `constrained` name or the fixed-point one.  Without it nothing of grow_interact.hip is touched.
  bool regularised = false, constrained = false, colsampled = false, interacting = false;
  GrowPairSplits reg_splits;
  uint32_t metric = kGrowMetricRmse;
  float slope = 1.0f;                  // delta of the pseudohuber metric, alpha of the quantile one
  // quantile (ohx_objective = quantile; then `pairs` holds too, the kind is Weighted or Sampled and splits() is null): the
  // pair path with grow_quantile.hip's pair kernel, the levels without the leaf kernel, the select that sets the leaves,
  // then the leaf kernel.  Without it, and without the quantile metric, nothing of grow_quantile.hip is touched.
  bool quantile = false;
  GrowQuantileArgs quantile_args;
  const GrowPairSplits* splits() const { return constrained || regularised || colsampled || interacting ? &reg_splits : nullptr; }
  bool wide() const { return which != Plain; }
  // The call's one plan, asked for once: the level loop over `cols` histogram columns - F itself, or the n_sel features
  // a tree of a sampled call sees (compact histograms and candidates) - the streaming kernels, which do not depend on
  // the columns, and the bin planes of all F features.
  GrowPlan plan(uint64_t n, uint32_t F, uint32_t cols, uint64_t ncuts, int max_depth, int num_cus) {
    GrowPlan p;
    if (which == Deep) {
      deep = plan_grow_deep_sampled(n, F, cols, ncuts, max_depth, num_cus);
      p = deep.lds;                    // the histograms of either path
      p.hist_bytes = std::max(p.hist_bytes, deep.scratch_bytes);
    } else {
      p = wide() ? plan_grow_weighted(n, cols, ncuts, max_depth, num_cus) : plan_grow(n, cols, ncuts, max_depth, num_cus);
    }
    p.bins_bytes = (uint64_t)F * n;    // the bins hold every feature
    return p;
  }
  // node records of one round, and the candidates of a level
  size_t node_stride() const { return which == Deep ? (size_t)deep.node_stride : (size_t)kGrowMaxNodes; }
  size_t best_count(uint32_t F, int max_depth) const {
    return which == Deep ? (size_t)(deep.best_bytes / sizeof(GrowCand)) : (size_t)(1u << (max_depth - 1)) * F;
  }
  hipError_t tree(const GrowArgs& a, const GrowPlan& plan, const GrowPlan& levels, uint32_t round, void* stream) const {
    switch (which) {
      case Deep: {
        GrowDeepArgs d = deep_args;
        d.g = a;
        return (hipError_t)(pairs ? launch_grow_tree_deep_pairs(d, pair_args, deep, round, h_state, stream, splits())
                                  : launch_grow_tree_deep(d, deep, round, h_state, stream));
      }
      case Sampled:
        if (quantile) return (hipError_t)launch_grow_tree_quantile(a, pair_args, quantile_args, plan, levels, round, stream);
        return (hipError_t)(pairs ? launch_grow_tree_pairs(a, pair_args, plan, levels, round, stream, splits())
                                  : launch_grow_tree_sampled(a, plan, levels, round, stream));
      case Weighted:
        if (quantile) return (hipError_t)launch_grow_tree_quantile(a, pair_args, quantile_args, plan, levels, round, stream);
        return (hipError_t)(pairs ? launch_grow_tree_pairs(a, pair_args, plan, levels, round, stream, splits())
                                  : launch_grow_tree_weighted(a, plan, levels, round, stream));
      default: return (hipError_t)launch_grow_tree(a, plan, levels, round, stream);
    }
  }
  hipError_t sse(const GrowEvalArgs& a, uint32_t blocks, uint32_t t, uint32_t set, void* stream) const {
    if (metric == kGrowMetricQuantile) return (hipError_t)launch_grow_sse_quantile(a, slope, blocks, t, set, stream);
    if (metric != kGrowMetricRmse) return (hipError_t)launch_grow_sse_metric(a, metric, slope, blocks, t, set, stream);
    return (hipError_t)(wide() ? launch_grow_sse_weighted(a, blocks, t, set, stream) : launch_grow_sse(a, blocks, t, set, stream));
  }
  hipError_t walk_sse(const GrowEvalArgs& a, uint32_t blocks, uint32_t round, uint32_t set, void* stream) const {
    if (metric == kGrowMetricQuantile)
      return (hipError_t)(which == Deep ? launch_grow_walk_sse_deep_quantile(a, deep_args, slope, blocks, round, set, stream)
                                        : launch_grow_walk_sse_quantile(a, slope, blocks, round, set, stream));
    if (metric != kGrowMetricRmse)
      return (hipError_t)(which == Deep ? launch_grow_walk_sse_deep_metric(a, deep_args, metric, slope, blocks, round, set, stream)
                                        : launch_grow_walk_sse_metric(a, metric, slope, blocks, round, set, stream));
    if (which == Deep) return (hipError_t)launch_grow_walk_sse_deep(a, deep_args, blocks, round, set, stream);
    return (hipError_t)(wide() ? launch_grow_walk_sse_weighted(a, blocks, round, set, stream)
                               : launch_grow_walk_sse(a, blocks, round, set, stream));
  }
  size_t words() const { return wide() ? 3 : 2; }
  size_t index(uint32_t t, uint32_t set) const { return wide() ? grow_wide_index(t, set) : grow_sum_index(t, set); }
  size_t count(size_t rounds) const { return wide() ? grow_wide_count(rounds) : grow_sum_count(rounds); }
  const char* sums_name() const { return wide() ? "the weighted metric sums" : "the metric sums"; }
  const char* hess_name() const { return wide() ? "the hessian histograms" : "the count histograms"; }
};

// Every OHXBoosterBoostTrees* entry point, in both forms.  The refusals that need neither a matrix nor a device come
// first, in the header's order; nothing is enqueued before the last of them.  Without `eval` nothing of the metric is
// allocated or enqueued; without `weights` nothing of the weights; without `sampling`, or with a subsample and a
// colsample_bytree of 1, nothing of the sampling: that call takes the weighted path.
void boost_trees(BoosterObj& b, const BoostCall& c) {
  const std::string w0(c.what);
  const char* what = c.what;
  const BoostEval& ev = c.eval;
  const BoostWeights& wt = c.weights;
  const bool weighted = wt.present, host_form = c.host_form;
  const int max_depth = c.max_depth;
  if (weighted && !ev.present) throw OhxError(w0 + ": the weighted call carries the metric");
  if (c.sampling.present && !weighted) throw OhxError(w0 + ": the sampled call carries the weights");
  if (c.deep && !weighted) throw OhxError(w0 + ": the deep call carries the weights");
  if (!b.loaded) throw OhxError("the booster holds no model: call XGBoosterLoadModel first");
  refuse_categorical(b, what);
  refuse_groups(b, what);
  if (!objective_is_identity(b.forest.objective))
    throw OhxError(w0 + " fits squared-error trees (gradient pred - label, hessian 1): the objective " + b.forest.objective +
                   " is not reg:squarederror");
  if (b.grow_objective != kGrowObjSquared && !weighted)
    throw OhxError(w0 + " keeps row counts, not hessian sums: with ohx_objective=" + grow_objective_name(b.grow_objective) +
                   " call OHXBoosterBoostTreesWeighted "
                   "(weights may be NULL) or a later form; nothing was enqueued and the forest is unchanged");
  if (b.grow_objective == kGrowObjQuantile) {
    // the leaves of a quantile tree are set by a select over per-leaf tables of 256 leaves, after the pair path's own splits
    const std::string tail = "; nothing was enqueued and the forest is unchanged";
    if (c.deep)
      throw OhxError(w0 + " keeps no per-leaf tables for the quantile leaves at any depth: with ohx_objective=quantile call "
                     "OHXBoosterBoostTreesWeighted or OHXBoosterBoostTreesSampled (max_depth <= 8), or set ohx_objective=squarederror" + tail);
    if (b.grow_alpha != 0.0f)
      throw OhxError(w0 + ": a quantile leaf honours no ohx_reg_alpha: set ohx_reg_alpha=0 or ohx_objective=squarederror" + tail);
    if (b.grow_max_delta_step != 0.0f)
      throw OhxError(w0 + ": a quantile leaf honours no ohx_max_delta_step: set ohx_max_delta_step=0 or ohx_objective=squarederror" + tail);
    if (!b.grow_mono.empty())
      throw OhxError(w0 + ": a quantile leaf honours no ohx_monotone_constraints: unset them (every entry 0) or set "
                     "ohx_objective=squarederror" + tail);
    if (b.grow_bylevel != 1.0f || b.grow_bynode != 1.0f)
      throw OhxError(w0 + ": ohx_objective=quantile grows with the pair path's own split kernels: set ohx_colsample_bylevel and "
                     "ohx_colsample_bynode to 1, or ohx_objective=squarederror" + tail);
  }
  if (!weighted && (b.grow_alpha != 0.0f || b.grow_max_delta_step != 0.0f || b.grow_metric != kGrowMetricRmse))
    throw OhxError(w0 + " keeps row counts and two-word sums: with ohx_reg_alpha, ohx_max_delta_step or ohx_eval_metric set call "
                   "OHXBoosterBoostTreesWeighted (weights may be NULL) or a later form; nothing was enqueued and the forest is unchanged");
  if (!weighted && !b.grow_mono.empty())
    throw OhxError(w0 + " keeps row counts, and its split kernels no weight intervals: with ohx_monotone_constraints active call "
                   "OHXBoosterBoostTreesWeighted (weights may be NULL) or a later form; nothing was enqueued and the forest is unchanged");
  if (!c.sampling.present && (b.grow_bylevel != 1.0f || b.grow_bynode != 1.0f))
    throw OhxError(w0 + " draws nothing and carries no seed: with ohx_colsample_bylevel or ohx_colsample_bynode below 1 call "
                   "OHXBoosterBoostTreesSampled or OHXBoosterBoostTreesDeepSampled, or set both to 1; nothing was enqueued and the "
                   "forest is unchanged");
  if (b.grow_mono.size() > (size_t)b.forest.num_feature)
    throw OhxError(w0 + ": ohx_monotone_constraints has " + std::to_string(b.grow_mono.size()) + " entries but the booster " +
                   std::to_string(b.forest.num_feature) + " features; nothing was enqueued and the forest is unchanged");
  // interaction constraints: the ids' range, then - while the groups take a candidate away from some node - what they do
  // not compose with (docs/35_interaction_constraints.md)
  const uint32_t ngroups = (uint32_t)(b.grow_interact.size() / 2);
  for (uint32_t f = b.forest.num_feature; f < kGrowMaxFeatures; ++f)
    for (uint32_t k = 0; k < ngroups; ++k)
      if (grow_interact_has(b.grow_interact.data() + 2 * k, f))
        throw OhxError(w0 + ": ohx_interaction_constraints names feature " + std::to_string(f) + " but the booster has " +
                       std::to_string(b.forest.num_feature) + " features; nothing was enqueued and the forest is unchanged");
  const bool interacting = b.forest.num_feature >= 1 && b.forest.num_feature <= kGrowMaxFeatures &&
                           grow_interact_active(b.grow_interact.data(), ngroups, b.forest.num_feature);
  if (interacting) {
    const std::string tail = "; nothing was enqueued and the forest is unchanged";
    if (!weighted)
      throw OhxError(w0 + " keeps row counts, and its split kernels no feature sets: with ohx_interaction_constraints active call "
                     "OHXBoosterBoostTreesWeighted (weights may be NULL) or a later form, or set it to []" + tail);
    if (b.grow_objective == kGrowObjQuantile)
      throw OhxError(w0 + ": ohx_objective=quantile grows with the pair path's own split kernels, which read no feature sets: set "
                     "ohx_interaction_constraints to [], or ohx_objective=squarederror" + tail);
  }
  if (!b.margin_error.empty()) throw OhxError(b.margin_error);
  if (c.labels == nullptr) throw OhxError(w0 + ": labels is NULL");
  if (c.cut_ptr == nullptr || c.cut_values == nullptr) throw OhxError(w0 + ": the cuts are NULL");
  const uint32_t F = b.forest.num_feature;
  if (F == 0 || F > kGrowMaxFeatures)
    throw OhxError(w0 + ": the booster has " + std::to_string(F) + " features; 1 to 128 are binned (their cuts are staged in LDS)");
  if (c.rounds < 1) throw OhxError(w0 + ": rounds must be >= 1");
  if (max_depth < 1 || max_depth > (c.deep ? kGrowDeepMaxDepth : kGrowMaxDepth))
    throw OhxError(w0 + (c.deep ? ": max_depth must be in 1..18" : ": max_depth must be in 1..8"));
  if (!std::isfinite(c.eta)) throw OhxError(w0 + ": eta must be finite");
  if (!(std::isfinite(c.lambda) && c.lambda >= 0.0f)) throw OhxError(w0 + ": lambda must be finite and >= 0");
  if (!(std::isfinite(c.gamma) && c.gamma >= 0.0f)) throw OhxError(w0 + ": gamma must be finite and >= 0");
  if (!weighted && c.min_child_rows < 1) throw OhxError(w0 + ": min_child_rows must be >= 1");
  if (weighted && !(std::isfinite(wt.min_child_weight) && wt.min_child_weight >= 0.0f))
    throw OhxError(w0 + ": min_child_weight must be finite and >= 0");
  uint32_t k_s = kGrowSampleOne, n_sel = F;   // the bag's threshold and the features a tree sees
  if (c.sampling.present) {
    k_s = grow_sample_threshold(c.sampling.subsample);
    if (k_s == 0)
      throw OhxError(w0 + ": subsample must be finite, > 0 and <= 1, and rint(subsample * 2^24) must be >= 1");
    n_sel = grow_num_selected(F, c.sampling.colsample_bytree);
    if (n_sel == 0) throw OhxError(w0 + ": colsample_bytree must be finite, > 0 and <= 1");
  }
  // the features a level sees of a tree's, and a node of a level's (the handle's fractions are sound: XGBoosterSetParam)
  uint32_t n_lvl = n_sel, n_node = n_sel;
  if (c.sampling.present) {
    n_lvl = grow_num_selected(n_sel, b.grow_bylevel);
    n_node = grow_num_selected(n_lvl, b.grow_bynode);
    if (n_lvl == 0 || n_node == 0) throw OhxError(w0 + ": ohx_colsample_bylevel and ohx_colsample_bynode must be finite, > 0 and <= 1");
  }
  if (interacting && (n_lvl != n_sel || n_node != n_lvl))
    throw OhxError(w0 + ": ohx_interaction_constraints is not crossed with the draws of ohx_colsample_bylevel and ohx_colsample_bynode: "
                   "set both to 1, or ohx_interaction_constraints to []; nothing was enqueued and the forest is unchanged");
  grow_check_cuts(c.cut_ptr, c.cut_values, F, what);
  if (ev.present) {
    if (ev.patience < 0) throw OhxError(w0 + ": patience must be >= 0");
    if (ev.rounds_run == nullptr || ev.best_round == nullptr) throw OhxError(w0 + ": rounds_run or best_round is NULL");
    if (ev.dmat == nullptr) {
      if (ev.patience >= 1)
        throw OhxError(w0 + ": patience " + std::to_string(ev.patience) + " needs a held-out matrix to stop on (eval_dmat is NULL)");
      if (ev.labels != nullptr || ev.nlabel != 0)
        throw OhxError(w0 + ": eval labels are given without a held-out matrix (eval_dmat is NULL)");
      if (wt.eval_weights != nullptr)
        throw OhxError(w0 + ": eval weights are given without a held-out matrix (eval_dmat is NULL)");
    } else if (ev.labels == nullptr) {
      throw OhxError(w0 + ": eval labels is NULL");
    }
  }
  DMatrixObj& d = *as_dmat(c.dmat);
  if (d.nrow == 0) throw OhxError(w0 + ": the matrix has no rows");
  if (c.nlabel != d.nrow) throw OhxError(w0 + ": " + std::to_string(c.nlabel) + " labels for " + std::to_string(d.nrow) + " rows");
  if (d.nrow > kRefitMaxRows) throw OhxError(w0 + ": at most 2^31 rows per call (" + std::to_string(d.nrow) + " given)");
  check_columns(b, d.ncol);
  DMatrixObj* e = nullptr;           // the held-out matrix
  if (ev.dmat != nullptr) {
    if (ev.dmat != c.dmat && !g_dmats.has(ev.dmat)) throw OhxError(w0 + ": the held-out DMatrix handle is invalid or has been freed");
    e = static_cast<DMatrixObj*>(ev.dmat);
    if (e->nrow == 0) throw OhxError(w0 + ": the held-out matrix has no rows");
    if (ev.nlabel != e->nrow)
      throw OhxError(w0 + ": " + std::to_string(ev.nlabel) + " eval labels for " + std::to_string(e->nrow) + " held-out rows");
    if (e->nrow > kRefitMaxRows) throw OhxError(w0 + ": at most 2^31 held-out rows per call (" + std::to_string(e->nrow) + " given)");
    check_columns(b, e->ncol);
    if (e->device >= 0 && d.device >= 0 && e->device != d.device)
      throw OhxError(w0 + ": the held-out DMatrix lives on HIP device " + std::to_string(e->device) + " but the training matrix on device " +
                     std::to_string(d.device));
  }
  // the kind of the call, once: everything below that differs by kernel or by sum layout asks `kind`
  // (a call whose fractions take no feature away is the call it is today, whatever the fractions)
  const bool colsampled = n_lvl != n_sel || n_node != n_lvl;
  const bool sampled = k_s != kGrowSampleOne || n_sel != F || colsampled;
  // (the Deep entry points at max_depth <= 8 take the weighted or the sampled kind as it is)
  const bool deep = c.deep && max_depth > kGrowMaxDepth;
  BoostKind kind{deep ? BoostKind::Deep : sampled ? BoostKind::Sampled : weighted ? BoostKind::Weighted : BoostKind::Plain};
  // (the Plain kind has no pair path: its hessian is a row count)
  kind.constrained = weighted && !b.grow_mono.empty();
  kind.regularised = weighted && !kind.constrained && (b.grow_alpha != 0.0f || b.grow_max_delta_step != 0.0f);
  kind.colsampled = colsampled;
  kind.interacting = interacting;
  kind.pairs = weighted && (b.grow_objective != kGrowObjSquared || b.grow_pairs_on || kind.regularised || kind.constrained || colsampled ||
                            interacting);
  if (kind.regularised && !colsampled && !interacting)
    kind.reg_splits = grow_reg_splits(GrowRegHess{(double)wt.min_child_weight, b.grow_alpha, b.grow_max_delta_step});
  kind.quantile = weighted && b.grow_objective == kGrowObjQuantile;
  kind.metric = weighted ? b.grow_metric : kGrowMetricRmse;
  kind.slope = kind.metric == kGrowMetricQuantile ? b.grow_quantile_alpha : b.grow_slope;
  kind.pair_args.objective = b.grow_objective;
  kind.pair_args.slope = kind.quantile ? b.grow_quantile_alpha : b.grow_slope;
  // before anything is built or enqueued: building the state waits for the library's stream
  if (!host_form && stream_capturing(c.caller))
    refuse_in_capture("grow trees", (w0 + " is not capturable; call it outside the capture").c_str());
  ensure_uploaded(b);                      // throws where there is no device; the initial margin is a margin predict
  const DeviceInfo dev = b.dev;
  check_same_device(d, dev.ordinal);
  if (e != nullptr) check_same_device(*e, dev.ordinal);
  if (!b.grow) b.grow = std::make_unique<GrowState>();
  GrowState& g = *b.grow;
  if (g.device != dev.ordinal) {
    g.release_device();                    // (what was left on another device)
    g.device = dev.ordinal;
  }
  if (!g.prepared) {
    HIP_CHECK((hipError_t)prepare_grow());
    g.prepared = true;
  }
  if (kind.pairs && !g.pairs_prepared) {
    HIP_CHECK((hipError_t)grow_lds_limits_pairs());
    g.pairs_prepared = true;
  }
  if (kind.quantile && !g.quantile_prepared) {
    HIP_CHECK((hipError_t)grow_lds_limits_quantile());
    g.quantile_prepared = true;
  }
  const uint64_t n = d.nrow, ncuts = c.cut_ptr[F];
  const size_t R = (size_t)c.rounds;
  // (n_sel == F where nothing is sampled, and n_lvl == n_sel where no level draws)
  const GrowPlan plan = kind.plan(n, F, n_lvl, ncuts, max_depth, dev.num_cus);
  const GrowPlan& levels = plan;
  const uint64_t tree0 = b.forest.trees.size();   // T0: tree t of the call is tree tree0 + t - 1 of the draws
  auto room = [&](auto& buf, size_t count, size_t elem, const char* name) {
    try {
      buf.ensure(count);
    } catch (const OhxError& e) {
      throw OhxError(w0 + ": " + name + " of " + std::to_string((uint64_t)count * elem) + " bytes cannot be allocated (" + e.what() + ")");
    }
  };
  const size_t nsums = kind.count(R);
  auto sums_room = [&]() {
    room(g.d_sums, nsums, 8, kind.sums_name());
    g.h_sums.ensure(nsums);
  };
  room(g.d_bins, (size_t)plan.bins_bytes, 1, "the bin planes (features x rows)");
  room(g.d_pos, n, 2, "the row positions");
  room(g.d_pred, n, 4, "the running margin");
  if (host_form) room(g.d_labels, n, 4, "the staged labels");
  room(g.d_Ghist, (size_t)(levels.hist_bytes / 16), 8, "the gradient histograms");
  room(g.d_Hhist, (size_t)(levels.hist_bytes / 16), 8, kind.hess_name());
  room(g.d_best, kind.best_count(F, max_depth), sizeof(GrowCand), "the split candidates");
  const size_t stride = kind.node_stride();
  room(g.d_nodes, R * stride, sizeof(GrowNode), "the node records");
  if (deep) {
    room(g.d_pos_deep, n, 4, "the row positions of the deep levels");
    if (e != nullptr) room(g.d_eval_nodes, stride * kGrowEvalNodeBytes, 1, "the held-out walk's node table");
  }
  const uint64_t ne = e != nullptr ? e->nrow : 0;
  GrowPlan eplan;                    // the held-out rows' binning
  if (weighted) {
    if (host_form && wt.weights != nullptr) room(g.d_weights, n, 4, "the staged weights");
    if (host_form && wt.eval_weights != nullptr) room(g.d_eval_weights, ne, 4, "the staged eval weights");
    sums_room();
  }
  if (kind.pairs) {
    room(g.d_pair_q, (size_t)(plan.pairs_bytes / kGrowPairRowBytes), 8, "the gradient plane of the pairs");
    room(g.d_pair_hq, (size_t)(plan.pairs_bytes / kGrowPairRowBytes), 4, "the hessian plane of the pairs");
    room(g.d_identity, F, 1, "the list of every feature");
    g.h_identity.ensure(F);
    for (uint32_t f = 0; f < F; ++f) g.h_identity.p[f] = (uint8_t)f;
  }
  if (kind.quantile) room(g.d_quantile, (size_t)kGrowQuantileBytes, 1, "the bins and the leaf table of the quantile select");
  if (kind.constrained) {
    room(g.d_mono_bounds, 2 * stride, 8, "the weight intervals of the monotone constraints");
    room(g.d_mono_constraints, F, 1, "the monotone constraints of every feature");
    g.h_mono_constraints.ensure(F);
    for (uint32_t f = 0; f < F; ++f) g.h_mono_constraints.p[f] = f < b.grow_mono.size() ? b.grow_mono[f] : (int8_t)0;
  }
  if (kind.interacting) {
    room(g.d_interact_sets, 4 * stride, 8, "the feature sets of the interaction constraints");
    room(g.d_interact_groups, 2 * (size_t)ngroups, 8, "the groups of the interaction constraints");
    g.h_interact_groups.ensure(2 * (size_t)ngroups);
    std::copy(b.grow_interact.begin(), b.grow_interact.end(), g.h_interact_groups.p);
  }
  const size_t bag_words = (size_t)((n + 63) / 64);
  if (sampled) {
    if (k_s != kGrowSampleOne) room(g.d_bag, bag_words, 8, "the bag's bit plane");
    room(g.d_features, R * n_sel, 1, "the selected features of every round");
    g.h_features.ensure(R * n_sel);
    // every round's list before anything is enqueued
    for (size_t r = 0; r < R; ++r)
      if (grow_pick_features(c.sampling.seed, tree0 + r, F, c.sampling.colsample_bytree, g.h_features.p + r * n_sel) != n_sel)
        throw OhxError(w0 + ": the selected features of round " + std::to_string(r + 1) + " are not " + std::to_string(n_sel));
  }
  const size_t level_bytes = R * (size_t)max_depth * n_lvl;
  if (colsampled) {
    room(g.d_level_lists, level_bytes, 1, "the level lists of every round");
    g.h_level_lists.ensure(level_bytes);
    // every round's and level's list before anything is enqueued
    for (size_t r = 0; r < R; ++r)
      for (uint32_t lv = 0; lv < (uint32_t)max_depth; ++lv)
        if (grow_pick_level_features(c.sampling.seed, tree0 + r, lv, g.h_features.p + r * n_sel, n_sel, b.grow_bylevel,
                                     g.h_level_lists.p + (r * (size_t)max_depth + lv) * n_lvl) != n_lvl)
          throw OhxError(w0 + ": the features of level " + std::to_string(lv) + " of round " + std::to_string(r + 1) + " are not " +
                         std::to_string(n_lvl));
  }
  if (ev.present) {
    if (e != nullptr) {
      eplan = plan_grow(ne, F, ncuts, std::min(max_depth, kGrowMaxDepth), dev.num_cus);
      room(g.d_eval_bins, (size_t)eplan.bins_bytes, 1, "the held-out bin planes (features x rows)");
      room(g.d_eval_pred, ne, 4, "the held-out margin");
      if (host_form) room(g.d_eval_labels, ne, 4, "the staged eval labels");
    }
    if (!weighted) sums_room();
  }
  g.d_tree_nodes.ensure(R);
  g.d_cuts.ensure(std::max<size_t>(ncuts, 1));
  g.d_cut_ptr.ensure(F + 1);
  g.d_state.ensure(1);
  g.d_saved_flag.ensure(1);
  if (!deep) g.h_nodes.ensure(R * kGrowMaxNodes);   // (the Deep kind sizes it by the records in use, at the end)
  g.h_tree_nodes.ensure(R);
  g.h_cuts.ensure(std::max<size_t>(ncuts, 1));
  g.h_cut_ptr.ensure(F + 1);
  g.h_state.ensure(1);
  for (uint32_t f = 0; f <= F; ++f) g.h_cut_ptr.p[f] = (uint32_t)c.cut_ptr[f];
  if (ncuts) memcpy(g.h_cuts.p, c.cut_values, ncuts * sizeof(float));
  hipStream_t stream = host_form ? lib_streams(dev.ordinal).exec : c.caller;
  if (host_form && (d.owned == nullptr || (e != nullptr && e->owned == nullptr))) order_behind_caller(dev.ordinal, stream);
  // The margin of the forest so far over the rows of `m`, by the predict path.  Its kernels raise the booster's sticky
  // inf flag for +-inf in a device matrix; bins take +-inf as the floats they are, so the flag word is put back as it was.
  auto initial_margin = [&](DMatrixObj& m, float* pred, uint64_t rows) {
    if (b.forest.trees.empty()) {
      uint32_t base_bits = 0;
      memcpy(&base_bits, &b.margin_base, sizeof base_bits);
      HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(pred), (int)base_bits, (size_t)rows, stream));
    } else {
      HIP_CHECK(hipMemcpyAsync(g.d_saved_flag.p, b.d_flags.p, sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
      launch_predict_checked(b, m, 1, 0, pred, stream);
      HIP_CHECK(hipMemcpyAsync(b.d_flags.p, g.d_saved_flag.p, sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    }
  };
  // every earlier call has been waited for, so the buffers are free
  HIP_CHECK(hipMemcpyAsync(g.d_cut_ptr.p, g.h_cut_ptr.p, (F + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  if (ncuts) HIP_CHECK(hipMemcpyAsync(g.d_cuts.p, g.h_cuts.p, ncuts * sizeof(float), hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipMemsetAsync(g.d_state.p, 0, sizeof(GrowLevelState), stream));
  HIP_CHECK(hipMemsetAsync(g.d_tree_nodes.p, 0, R * sizeof(uint32_t), stream));
  HIP_CHECK(hipMemsetAsync(g.d_pos.p, 0, n * sizeof(uint16_t), stream));
  if (deep) HIP_CHECK(hipMemsetAsync(g.d_pos_deep.p, 0, n * sizeof(uint32_t), stream));
  if (sampled) HIP_CHECK(hipMemcpyAsync(g.d_features.p, g.h_features.p, R * n_sel, hipMemcpyHostToDevice, stream));
  if (colsampled) HIP_CHECK(hipMemcpyAsync(g.d_level_lists.p, g.h_level_lists.p, level_bytes, hipMemcpyHostToDevice, stream));
  if (kind.pairs) HIP_CHECK(hipMemcpyAsync(g.d_identity.p, g.h_identity.p, F, hipMemcpyHostToDevice, stream));
  if (kind.constrained) HIP_CHECK(hipMemcpyAsync(g.d_mono_constraints.p, g.h_mono_constraints.p, F, hipMemcpyHostToDevice, stream));
  if (kind.interacting)
    HIP_CHECK(hipMemcpyAsync(g.d_interact_groups.p, g.h_interact_groups.p, 2 * (size_t)ngroups * sizeof(uint64_t), hipMemcpyHostToDevice,
                             stream));
  if (host_form) HIP_CHECK(hipMemcpyAsync(g.d_labels.p, c.labels, n * sizeof(float), hipMemcpyHostToDevice, stream));
  initial_margin(d, g.d_pred.p, n);
  if (ev.present) HIP_CHECK(hipMemsetAsync(g.d_sums.p, 0, nsums * sizeof(unsigned long long), stream));
  if (host_form && wt.weights != nullptr)
    HIP_CHECK(hipMemcpyAsync(g.d_weights.p, wt.weights, n * sizeof(float), hipMemcpyHostToDevice, stream));
  if (host_form && wt.eval_weights != nullptr)
    HIP_CHECK(hipMemcpyAsync(g.d_eval_weights.p, wt.eval_weights, ne * sizeof(float), hipMemcpyHostToDevice, stream));
  if (e != nullptr) {
    // the held-out rows get what the training rows got: staged labels, and the margin of the forest so far
    if (host_form) HIP_CHECK(hipMemcpyAsync(g.d_eval_labels.p, ev.labels, ne * sizeof(float), hipMemcpyHostToDevice, stream));
    initial_margin(*e, g.d_eval_pred.p, ne);
  }
  // a weight array as the kernels read it: the staged copy, the caller's device array, or nullptr (all 1.0f)
  auto device_weights = [&](const float* given, DevBuf<float>& staged) {
    return given == nullptr ? nullptr : host_form ? staged.p : given;
  };
  GrowArgs a;
  a.rows = d.d_data;
  a.nrow = n;
  a.ncol = (uint32_t)d.ncol;
  a.num_feature = F;
  a.missing = d.missing;
  a.labels = host_form ? g.d_labels.p : c.labels;
  a.cut_ptr = g.d_cut_ptr.p;
  a.cuts = g.d_cuts.p;
  a.ncuts = (uint32_t)ncuts;
  a.bins = g.d_bins.p;
  a.pos = g.d_pos.p;
  a.pred = g.d_pred.p;
  a.Ghist = g.d_Ghist.p;
  a.Hhist = g.d_Hhist.p;
  a.best = g.d_best.p;
  a.nodes = g.d_nodes.p;
  a.tree_nodes = g.d_tree_nodes.p;
  a.state = g.d_state.p;
  a.max_depth = max_depth;
  a.eta = c.eta;
  a.lambda = c.lambda;
  a.gamma = c.gamma;
  a.min_child_rows = c.min_child_rows;
  a.weights = device_weights(wt.weights, g.d_weights);
  a.min_child_weight = (double)wt.min_child_weight;
  if (sampled) {                       // a bag of the rows and a tree's features
    a.bag = k_s != kGrowSampleOne ? g.d_bag.p : nullptr;
    a.features = g.d_features.p;
    a.n_sel = n_sel;
    a.k_s = k_s;
  }
  if (kind.pairs) {
    kind.pair_args.q = g.d_pair_q.p;
    kind.pair_args.hq = g.d_pair_hq.p;
    kind.pair_args.identity = g.d_identity.p;
  }
  if (kind.quantile) {
    kind.quantile_args.hist = reinterpret_cast<unsigned long long*>(g.d_quantile.p);
    kind.quantile_args.state = reinterpret_cast<GrowQuantileState*>(g.d_quantile.p + kGrowQuantileHistBytes);
    kind.quantile_args.hq = g.d_pair_hq.p;
    kind.quantile_args.alpha = b.grow_quantile_alpha;
  }
  if (colsampled) {
    GrowColsampleArgs cs;
    cs.lists = g.d_level_lists.p;
    cs.depth = (uint32_t)max_depth;
    cs.n_lvl = n_lvl;
    cs.n_node = n_node;
    cs.seed = c.sampling.seed;
    cs.tree0 = tree0;
    const GrowRegHess reg{(double)wt.min_child_weight, b.grow_alpha, b.grow_max_delta_step};
    kind.reg_splits = kind.constrained    ? grow_colsample_splits(cs, GrowMonoArgs{reg, g.d_mono_bounds.p, g.d_mono_constraints.p})
                      : kind.regularised ? grow_colsample_splits(cs, reg)
                                         : grow_colsample_splits(cs, GrowFixedHess{(double)wt.min_child_weight});
  } else if (kind.interacting) {
    const GrowRegHess reg{(double)wt.min_child_weight, b.grow_alpha, b.grow_max_delta_step};
    const uint64_t* groups = g.d_interact_groups.p;
    uint64_t* sets = g.d_interact_sets.p;
    kind.reg_splits =
        kind.constrained ? grow_interact_splits(GrowInteractArgs<GrowMonoArgs>{groups, sets, ngroups,
                                                                               GrowMonoArgs{reg, g.d_mono_bounds.p, g.d_mono_constraints.p}})
        : kind.regularised ? grow_interact_splits(GrowInteractArgs<GrowRegHess>{groups, sets, ngroups, reg})
                           : grow_interact_splits(GrowInteractArgs<GrowFixedHess>{groups, sets, ngroups,
                                                                                 GrowFixedHess{(double)wt.min_child_weight}});
  } else if (kind.constrained) {
    kind.reg_splits = grow_mono_splits(GrowMonoArgs{GrowRegHess{(double)wt.min_child_weight, b.grow_alpha, b.grow_max_delta_step},
                                                    g.d_mono_bounds.p, g.d_mono_constraints.p});
  }
  if (deep) {
    kind.deep_args.pos = g.d_pos_deep.p;
    kind.deep_args.node_stride = (uint32_t)stride;
    kind.deep_args.eval_nodes = e != nullptr ? g.d_eval_nodes.p : nullptr;
    kind.deep_args.g = a;              // (the walk launcher reads the records and their counts from it)
    kind.h_state = g.h_state.p;
  }
  // one tree by the kernels of the call's kind
  auto grow_tree = [&](uint32_t r) {
    if (a.bag != nullptr) {
      a.row_key = grow_row_key(c.sampling.seed, tree0 + r);
      const hipError_t drawn = (hipError_t)launch_grow_bag(a, plan, stream);
      if (drawn != hipSuccess) return drawn;
    }
    return kind.tree(a, plan, levels, r, stream);
  };
  hipError_t launched = (hipError_t)launch_grow_bin(a, plan, stream);
  hipError_t waited = hipSuccess;
  uint32_t run = (uint32_t)c.rounds, best = 0;   // rounds grown, and the best of them by the held-out sums
  // the held-out sum after t trees as the exact integer, from the host copy of the sums
  auto held = [&](uint32_t t) { return grow_sum_value(g.h_sums.p + kind.index(t, kGrowEvalHeldOut), kind.words()); };
  std::vector<unsigned __int128> S(ev.present ? R + 1 : 0);   // the held-out sums, as far as they are known
  if (!ev.present) {
    for (uint32_t r = 0; launched == hipSuccess && r < (uint32_t)c.rounds; ++r) launched = grow_tree(r);
  } else {
    // the metric: the training rows' sums after every leaf kernel, the held-out rows' walk of every new tree, and both
    // sets' sums of the forest as loaded
    GrowEvalArgs mt;
    mt.pred = g.d_pred.p;
    mt.labels = a.labels;
    mt.nrow = n;
    mt.num_feature = F;
    mt.nodes = g.d_nodes.p;
    mt.tree_nodes = g.d_tree_nodes.p;
    mt.sums = mt.wsums = g.d_sums.p;   // (a kind's kernels read the one of its layout)
    mt.state = g.d_state.p;
    mt.max_depth = max_depth;
    mt.label_flag = kGrowFlagLabel;
    mt.weights = a.weights;
    mt.weight_flag = kGrowFlagWeight;
    GrowEvalArgs me = mt;
    const uint32_t tblocks = plan_grow_eval_blocks(n, dev.num_cus);
    uint32_t eblocks = 0;
    if (e != nullptr) {
      GrowArgs ab = a;               // the binning alone, on the held-out arrays and the same staged cuts
      ab.rows = e->d_data;
      ab.nrow = ne;
      ab.ncol = (uint32_t)e->ncol;
      ab.missing = e->missing;
      ab.labels = nullptr;
      ab.bins = g.d_eval_bins.p;
      ab.pos = nullptr;
      ab.pred = nullptr;
      if (launched == hipSuccess) launched = (hipError_t)launch_grow_bin(ab, eplan, stream);
      me.bins = g.d_eval_bins.p;
      me.pred = g.d_eval_pred.p;
      me.labels = host_form ? g.d_eval_labels.p : ev.labels;
      me.nrow = ne;
      me.label_flag = kGrowFlagEvalLabel;
      me.weights = device_weights(wt.eval_weights, g.d_eval_weights);
      me.weight_flag = kGrowFlagEvalWeight;
      eblocks = plan_grow_eval_blocks(ne, dev.num_cus);
    }
    auto sum_train = [&](uint32_t t) { return kind.sse(mt, tblocks, t, kGrowEvalTrain, stream); };
    if (launched == hipSuccess && e != nullptr) launched = kind.sse(me, eblocks, 0, kGrowEvalHeldOut, stream);
    if (launched == hipSuccess) launched = sum_train(0);
    const bool stepwise = ev.patience >= 1;
    for (uint32_t r = 0; launched == hipSuccess && waited == hipSuccess && r < (uint32_t)c.rounds; ++r) {
      launched = grow_tree(r);
      if (launched == hipSuccess) launched = sum_train(r + 1);
      if (launched == hipSuccess && e != nullptr) launched = kind.walk_sse(me, eblocks, r, kGrowEvalHeldOut, stream);
      if (!stepwise || launched != hipSuccess) continue;
      // one small wait a round: this round's held-out sums (and round 0's, the first time) and the error word
      const uint32_t t0 = r == 0 ? 0 : r + 1;
      for (uint32_t t = t0; launched == hipSuccess && t <= r + 1; ++t) {
        const size_t at = kind.index(t, kGrowEvalHeldOut);
        launched = hipMemcpyAsync(g.h_sums.p + at, g.d_sums.p + at, kind.words() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream);
      }
      if (launched == hipSuccess) launched = hipMemcpyAsync(g.h_state.p, g.d_state.p, sizeof(GrowLevelState), hipMemcpyDeviceToHost, stream);
      if (launched != hipSuccess) break;
      waited = hipStreamSynchronize(stream);
      if (waited != hipSuccess) break;
      if (g.h_state.p->error != 0) {   // refused below; nothing more is enqueued
        run = r + 1;
        break;
      }
      for (uint32_t t = t0; t <= r + 1; ++t) S[t] = held(t);
      best = grow_eval_best(S.data(), best, r + 1);
      if (grow_eval_stops(best, r + 1, ev.patience)) {
        run = r + 1;
        break;
      }
    }
    if (launched == hipSuccess && waited == hipSuccess)
      launched = hipMemcpyAsync(g.h_sums.p, g.d_sums.p, nsums * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream);
  }
  if (launched == hipSuccess && !deep)
    launched = hipMemcpyAsync(g.h_nodes.p, g.d_nodes.p, R * kGrowMaxNodes * sizeof(GrowNode), hipMemcpyDeviceToHost, stream);
  if (launched == hipSuccess) launched = hipMemcpyAsync(g.h_tree_nodes.p, g.d_tree_nodes.p, R * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
  if (launched == hipSuccess) launched = hipMemcpyAsync(g.h_state.p, g.d_state.p, sizeof(GrowLevelState), hipMemcpyDeviceToHost, stream);
  // both forms wait, whatever was enqueued: the labels and the records are read from the caller's and the state's memory
  hipError_t waited_last = hipStreamSynchronize(stream);
  // the Deep kind: the counts first, then only the records in use, packed round after round
  std::vector<size_t> first(R + 1, 0);
  if (deep && launched == hipSuccess && waited == hipSuccess && waited_last == hipSuccess && g.h_state.p->error == 0) {
    for (size_t r = 0; r < R; ++r) first[r + 1] = first[r] + std::min<size_t>(g.h_tree_nodes.p[r], stride);
    g.h_nodes.ensure(std::max<size_t>(first[R], 1));
    for (size_t r = 0; launched == hipSuccess && r < R; ++r)
      if (first[r + 1] != first[r])
        launched = hipMemcpyAsync(g.h_nodes.p + first[r], g.d_nodes.p + r * stride, (first[r + 1] - first[r]) * sizeof(GrowNode),
                                  hipMemcpyDeviceToHost, stream);
    waited_last = hipStreamSynchronize(stream);
  }
  if (!host_form) {
    d.used_async = true;
    if (e != nullptr) e->used_async = true;
  }
  HIP_CHECK(launched);
  HIP_CHECK(waited);
  HIP_CHECK(waited_last);
  const uint32_t flags = g.h_state.p->error;
  if (flags & kGrowFlagLabel)
    throw OhxError(w0 + ": a gradient pred - label is not finite or reaches 256 in size at some row and round: look for a "
                   "label that is NaN, infinite or far from the model's range; the forest is unchanged");
  if (flags & kGrowFlagEvalLabel)
    throw OhxError(w0 + ": a held-out residual pred - eval label is not finite or reaches 256 in size at some row and round: "
                   "look for an eval label that is NaN, infinite or far from the model's range; the forest is unchanged");
  if (flags & kGrowFlagWeight)
    throw OhxError(w0 + ": a weight is not finite, is negative or reaches 256 at some training row; the forest is unchanged");
  if (flags & kGrowFlagEvalWeight)
    throw OhxError(w0 + ": an eval weight is not finite, is negative or reaches 256 at some held-out row; the forest is unchanged");
  if (flags & kGrowFlagHess)
    throw OhxError(w0 + ": the root of some round holds no hessian (every in-bag rint(h * w * 2^24) is 0: the residuals are far "
                   "beyond ohx_huber_slope, the weights are 0, or no row was drawn); raise ohx_huber_slope; the forest is unchanged");
  if (flags & kGrowFlagBag)
    throw OhxError(w0 + ": the bag of some round holds no weight (every row drawn by subsample has rint(w * 2^24) == 0, or none "
                   "was drawn): raise subsample or change the seed; the forest is unchanged");
  if (flags != 0) throw OhxError(w0 + ": the grow kernels reported error flags " + std::to_string(flags));
  if (weighted) {                      // W of both sets leads the wide sums
    if (g.h_sums.p[kGrowEvalTrain] == 0ull)
      throw OhxError(w0 + ": the weights of the training rows sum to 0 (every rint(w * 2^24) is 0); the forest is unchanged");
    if (e != nullptr && g.h_sums.p[kGrowEvalHeldOut] == 0ull)
      throw OhxError(w0 + ": the eval weights of the held-out rows sum to 0 (every rint(w * 2^24) is 0); the forest is unchanged");
  }
  // all or nothing: every round is done and the error word is clean
  size_t keep = R;                     // the trees that are appended
  if (ev.present) {
    if (e != nullptr) {
      // the shared rule over the whole list, from the exact integers: what the round-by-round loop decided
      uint32_t run_again = 0;
      for (uint32_t t = 0; t <= run; ++t) S[t] = held(t);
      grow_eval_stop(S.data(), run, ev.patience, &run_again, &best);
      if (run_again != run) throw OhxError(w0 + ": the stop rule gave " + std::to_string(run_again) + " rounds over the sums of " + std::to_string(run));
      if (ev.patience >= 1) keep = best;
    } else {
      best = run;
    }
  }
  std::vector<Tree> grown;
  bst_ulong added = 0;
  for (size_t r = 0; r < keep; ++r) {
    grown.push_back(grow_assemble_tree(g.h_nodes.p + (deep ? first[r] : r * kGrowMaxNodes), g.h_tree_nodes.p[r], F, (uint32_t)stride));
    added += g.h_tree_nodes.p[r];
  }
  const size_t T0 = (size_t)tree0;
  for (Tree& t : grown) {
    b.forest.trees.push_back(std::move(t));
    b.forest.tree_info.push_back(0);
  }
  try {
    b.forest.validate();
  } catch (...) {
    b.forest.trees.resize(T0);
    b.forest.tree_info.resize(T0);
    throw;
  }
  // everything built from the forest is dropped as a model load drops it; the leaf numbering has changed, so the visit
  // state goes with its counters.  No tree kept (best == 0): the forest and everything built from it stay.
  if (keep != 0) {
    invalidate_device_state(b);
    b.contribs.reset();
    drop_leaf_walk(b);
  }
  if (c.nodes_added != nullptr) *c.nodes_added = added;
  if (ev.present) {
    // the RMSE of sum (t, set): the wide sum over the set's W, or the plain sum over the set's rows
    auto rmse = [&](uint32_t t, uint32_t set) {
      const unsigned long long* s = g.h_sums.p + kind.index(t, set);
      if (weighted) {
        GrowWideSum x;
        x.p2 = s[0];
        x.p1 = s[1];
        x.p0 = s[2];
        return kind.metric == kGrowMetricRmse       ? grow_wide_rmse(x, g.h_sums.p[set])
               : kind.metric == kGrowMetricQuantile ? grow_wide_quantile(x, g.h_sums.p[set])
                                                    : grow_wide_mean(x, g.h_sums.p[set]);
      }
      GrowSum x;
      x.hi = s[0];
      x.lo = s[1];
      return grow_sum_rmse(x, set == kGrowEvalTrain ? n : ne);
    };
    for (uint32_t t = 0; t <= run; ++t) {
      if (ev.train_rmse != nullptr) ev.train_rmse[t] = rmse(t, kGrowEvalTrain);
      if (ev.eval_rmse != nullptr && e != nullptr) ev.eval_rmse[t] = rmse(t, kGrowEvalHeldOut);
    }
    *ev.rounds_run = (int)run;
    *ev.best_round = (int)best;
  }
}

// ---- quantile cuts from rows in HBM (cuts.hpp) ----

// OHXDMatrixQuantileCuts.  The refusals that need neither a matrix nor a device come first; nothing is enqueued before
// the last refusal.  The scratch is this call's own: allocated on the matrix's device and freed before it returns.
void dmatrix_quantile_cuts(DMatrixHandle dmat, bst_ulong row_step, int max_bins, bst_ulong* cut_ptr, float* cut_values,
                           bst_ulong cap, bst_ulong* needed, hipStream_t stream) {
  const std::string w0("OHXDMatrixQuantileCuts");
  if (cut_ptr == nullptr || needed == nullptr) throw OhxError(w0 + ": NULL output argument");
  if (cut_values == nullptr && cap != 0) throw OhxError(w0 + ": cut_values is NULL");
  if (max_bins < 2 || max_bins > (int)kCutsMaxBins) throw OhxError(w0 + ": max_bins must be in 2..255");
  if (row_step < 1) throw OhxError(w0 + ": row_step must be >= 1");
  DMatrixObj& d = *as_dmat(dmat);
  if (d.nrow > kCutsMaxRows) throw OhxError(w0 + ": at most 2^31 rows per call (" + std::to_string(d.nrow) + " given)");
  static_assert(sizeof(bst_ulong) == sizeof(uint64_t), "bst_ulong is uint64");
  uint64_t* ptr = reinterpret_cast<uint64_t*>(cut_ptr);
  const uint64_t ncol = d.ncol;
  if (d.nrow == 0 || ncol == 0) {        // nothing to look at: no cuts, and nothing is launched
    for (uint64_t c = 0; c <= ncol; ++c) ptr[c] = 0;
    *needed = 0;
    return;
  }
  if (ncol > 0xFFFFFFFFull) throw OhxError(w0 + ": " + std::to_string(ncol) + " columns");
  const DeviceInfo dev = use_device(d.device);       // throws where there is no device
  if (stream_capturing(stream)) refuse_in_capture("make quantile cuts", (w0 + " is not capturable; call it outside the capture").c_str());
  HIP_CHECK((hipError_t)prepare_cuts());
  const CutsPlan plan = plan_cuts(d.nrow, row_step, ncol, dev.num_cus);
  DevBuf<uint32_t> d_table1, d_table;
  DevBuf<CutsCol> d_cols;
  PinnedBuf<CutsCol> h_cols;
  auto room = [&](auto& buf, size_t count, size_t elem, const char* name) {
    try {
      buf.ensure(count);
    } catch (const OhxError& e) {
      throw OhxError(w0 + ": " + name + " of " + std::to_string((uint64_t)count * elem) + " bytes cannot be allocated (" + e.what() + ")");
    }
  };
  room(d_table1, (size_t)(plan.table1_bytes / 4), 4, "the first pass's counters (columns x 4096)");
  room(d_table, (size_t)(plan.table_bytes / 4), 4, "the later passes' counters (columns x 255 x 1024)");
  room(d_cols, (size_t)ncol, sizeof(CutsCol), "the column records");
  room(h_cols, (size_t)ncol, sizeof(CutsCol), "the host copy of the column records");
  CutsArgs a;
  a.rows = d.d_data;
  a.sampled = plan.sampled;
  a.row_step = row_step;
  a.ncol = (uint32_t)ncol;
  a.missing = d.missing;
  a.max_bins = (uint32_t)max_bins;
  a.table1 = d_table1.p;
  a.table = d_table.p;
  a.cols = d_cols.p;
  hipError_t launched = (hipError_t)launch_cuts(a, plan, stream);
  if (launched == hipSuccess) launched = hipMemcpyAsync(h_cols.p, d_cols.p, (size_t)ncol * sizeof(CutsCol), hipMemcpyDeviceToHost, stream);
  // the one wait, whatever was enqueued: the scratch is freed on return
  const hipError_t waited = hipStreamSynchronize(stream);
  HIP_CHECK(launched);
  HIP_CHECK(waited);
  *needed = cuts_write(h_cols.p, ncol, (uint32_t)max_bins, ptr, cut_values, cap);
  if (*needed > cap)
    throw OhxError(w0 + ": " + std::to_string(*needed) + " cut values are needed and cut_values holds " + std::to_string(cap));
}

}  // namespace

// =================================================================== C ABI

#pragma GCC visibility push(default)
extern "C" {

const char* XGBGetLastError(void) { return g_last_error.c_str(); }

int OHXDeviceCount(int* out) {
  API_BEGIN();
  if (out == nullptr) throw OhxError("OHXDeviceCount: out is NULL");
  *out = device_count_or_throw();
  API_END();
}

int XGDMatrixCreateFromMat(const float* data, bst_ulong nrow, bst_ulong ncol, float missing, DMatrixHandle* out) {
  API_BEGIN();
  if (out == nullptr) throw OhxError("XGDMatrixCreateFromMat: out is NULL");
  if (data == nullptr && nrow * ncol != 0) throw OhxError("XGDMatrixCreateFromMat: data is NULL");
  DeviceInfo dev = use_device(-1);
  auto d = std::make_unique<DMatrixObj>();
  d->nrow = nrow;
  d->ncol = ncol;
  d->missing = missing;
  d->device = dev.ordinal;
  const size_t count = (size_t)nrow * (size_t)ncol;
  d->owned = g_row_pool.take(count, dev.ordinal, &d->owned_cap);
  d->d_data = d->owned;
  if (count) {
    // two waits per call: the copy itself (pageable host memory) and one read-back of the inf flag
    hipStream_t s = lib_streams(dev.ordinal).exec;
    HIP_CHECK(hipMemcpyAsync(d->owned, data, count * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));          // `data` is the caller's again (:383 deallocates it)
    // xgboost 1.6.0 (SparsePage::Push): "Input data contains `inf` or `nan`"
    std::lock_guard<std::mutex> g(g_check.mu);
    g_check.ensure(1, dev.ordinal);
    HIP_CHECK(hipMemsetAsync(g_check.d.p, 0, sizeof(uint32_t), s));
    HIP_CHECK(launch_scan_dense(d->owned, count, missing, g_check.d.p, s));
    HIP_CHECK(hipMemcpyAsync(g_check.h.p, g_check.d.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (g_check.h.p[0] & kFlagInfInput) throw OhxError("Input data contains `inf` or `nan`");
  }
  g_dmats.add(d.get());
  *out = d.release();
  API_END();
}

int OHXDMatrixGetGrid(DMatrixHandle handle, int* im, int* jm, bst_ulong* row0, int* inferred) {
  API_BEGIN();
  DMatrixObj* d = as_dmat(handle);
  // a matrix the library copied itself can be searched whenever it is asked about
  if (d->owned != nullptr && !d->grid_looked && d->grid_im == 0) {
    HIP_CHECK(hipSetDevice(d->device));
    infer_level_size(*d, lib_streams(d->device).exec);
  }
  if (im) *im = d->grid_im;
  if (jm) *jm = d->grid_jm;
  if (row0) *row0 = d->grid_row0;
  if (inferred) *inferred = d->grid_inferred ? 1 : 0;
  API_END();
}

int OHXDMatrixInferGrid(DMatrixHandle handle, void* stream, int* found) {
  API_BEGIN();
  DMatrixObj* d = as_dmat(handle);
  HIP_CHECK(hipSetDevice(d->device));
  d->grid_im = d->grid_jm = 0;
  d->grid_row0 = 0;
  d->grid_inferred = false;
  infer_level_size(*d, static_cast<hipStream_t>(stream));   // waits for `stream`: the rows must be there
  if (found) *found = d->grid_inferred ? 1 : 0;
  API_END();
}

int OHXDMatrixCreateFromDevice(const float* d_data, bst_ulong nrow, bst_ulong ncol, float missing, DMatrixHandle* out) {
  API_BEGIN();
  if (out == nullptr) throw OhxError("OHXDMatrixCreateFromDevice: out is NULL");
  if (d_data == nullptr && nrow * ncol != 0) throw OhxError("OHXDMatrixCreateFromDevice: d_data is NULL");
  DeviceInfo dev = use_device(-1);
  auto d = std::make_unique<DMatrixObj>();
  d->nrow = nrow;
  d->ncol = ncol;
  d->missing = missing;
  d->d_data = d_data;
  d->device = dev.ordinal;
  g_dmats.add(d.get());
  *out = d.release();
  API_END();
}

int OHXDMatrixSetGrid(DMatrixHandle handle, int im, int jm, bst_ulong row0) {
  API_BEGIN();
  DMatrixObj* d = as_dmat(handle);
  if (im < 0 || jm < 0 || (im == 0) != (jm == 0)) throw OhxError("OHXDMatrixSetGrid: im and jm must both be positive (or both 0)");
  d->grid_im = im;
  d->grid_jm = jm;
  d->grid_row0 = im ? row0 : 0;
  d->grid_inferred = false;
  d->grid_looked = true;          // the caller has spoken (0, 0 = "no grid": 64 consecutive rows per wave)
  API_END();
}

int XGDMatrixFree(DMatrixHandle handle) {
  API_BEGIN();
  if (handle == nullptr || !g_dmats.remove(handle)) throw OhxError("DMatrix handle is invalid or has been freed");
  delete static_cast<DMatrixObj*>(handle);
  API_END();
}

int OHXReleaseScratch(void);   // defined at the end of the file: it knows every pool

int XGDMatrixNumRow(DMatrixHandle handle, bst_ulong* out) {
  API_BEGIN();
  if (out == nullptr) throw OhxError("XGDMatrixNumRow: out is NULL");
  *out = as_dmat(handle)->nrow;
  API_END();
}

int XGDMatrixNumCol(DMatrixHandle handle, bst_ulong* out) {
  API_BEGIN();
  if (out == nullptr) throw OhxError("XGDMatrixNumCol: out is NULL");
  *out = as_dmat(handle)->ncol;
  API_END();
}

int XGDMatrixSaveBinary(DMatrixHandle handle, const char* fname, int silent) {
  API_BEGIN();
  (void)silent;
  DMatrixObj* d = as_dmat(handle);
  if (fname == nullptr) throw OhxError("XGDMatrixSaveBinary: fname is NULL");
  const size_t count = (size_t)d->nrow * (size_t)d->ncol;
  std::vector<float> host(count);
  if (count) {
    HIP_CHECK(hipSetDevice(d->device));
    hipStream_t st = lib_streams(d->device).exec;
    if (d->owned == nullptr) order_behind_caller(d->device, st);
    HIP_CHECK(hipMemcpyAsync(host.data(), d->d_data, count * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }
  std::ofstream o(fname, std::ios::binary);
  if (!o) throw OhxError(std::string("cannot open '") + fname + "' for writing");
  o.write("OHXDMAT1", 8);
  o.write((const char*)&d->nrow, 8);
  o.write((const char*)&d->ncol, 8);
  o.write((const char*)&d->missing, 4);
  o.write((const char*)host.data(), (std::streamsize)(count * sizeof(float)));
  if (!o) throw OhxError(std::string("failed writing '") + fname + "'");
  API_END();
}

int XGDMatrixCreateFromFile(const char* fname, int silent, DMatrixHandle* out) {
  API_BEGIN();
  (void)silent;
  if (fname == nullptr || out == nullptr) throw OhxError("XGDMatrixCreateFromFile: NULL argument");
  std::string uri(fname), path(fname);
  bool csv = false;
  size_t q = uri.find('?');
  if (q != std::string::npos) {
    path = uri.substr(0, q);
    csv = uri.find("format=csv", q) != std::string::npos;
  }
  if (ends_with(path, ".csv")) csv = true;
  std::ifstream in(path, std::ios::binary);
  if (!in) throw OhxError("cannot open '" + path + "'");
  std::vector<float> host;
  uint64_t nrow = 0, ncol = 0;
  float missing = NAN;
  if (csv) {
    std::string line;
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      uint64_t c = 0;
      std::stringstream ss(line);
      std::string cell;
      while (std::getline(ss, cell, ',')) {
        host.push_back(cell.empty() ? NAN : strtof(cell.c_str(), nullptr));
        ++c;
      }
      if (ncol == 0) ncol = c;
      if (c != ncol) throw OhxError("CSV '" + path + "': ragged row " + std::to_string(nrow));
      ++nrow;
    }
  } else {
    char magic[8];
    in.read(magic, 8);
    if (!in || memcmp(magic, "OHXDMAT1", 8) != 0)
      throw OhxError("'" + path + "' is not a dense matrix saved by XGDMatrixSaveBinary of this library "
                     "(xgboost's own binary DMatrix cache and libsvm text are not supported)");
    in.read((char*)&nrow, 8);
    in.read((char*)&ncol, 8);
    in.read((char*)&missing, 4);
    host.resize((size_t)nrow * (size_t)ncol);
    in.read((char*)host.data(), (std::streamsize)(host.size() * sizeof(float)));
    if (!in) throw OhxError("'" + path + "' is truncated");
  }
  int rc = XGDMatrixCreateFromMat(host.data(), nrow, ncol, missing, out);
  if (rc != 0) throw OhxError(g_last_error);
  API_END();
}

int XGBoosterCreate(const DMatrixHandle dmats[], bst_ulong len, BoosterHandle* out) {
  API_BEGIN();
  if (out == nullptr) throw OhxError("XGBoosterCreate: out is NULL");
  // The reference passes one handle BY VALUE with len == 0 (OH_GridCompMod.F90:255-256):
  // with len == 0 the pointer is not an array and must not be read.
  for (bst_ulong i = 0; i < len; ++i) (void)as_dmat(dmats[i]);
  auto* b = new BoosterObj();
  g_boosters.add(b);
  *out = b;
  API_END();
}

int XGBoosterFree(BoosterHandle handle) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  if (!g_boosters.remove(handle)) throw OhxError("Booster handle is invalid or has been freed");
  if (b->uploaded) (void)hipSetDevice(b->dev.ordinal);
  delete b;
  API_END();
}

int XGBoosterLoadModel(BoosterHandle handle, const char* fname) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  if (fname == nullptr) throw OhxError("XGBoosterLoadModel: fname is NULL");
  adopt_model(*b, load_model_file(fname));
  API_END();
}

int XGBoosterLoadModelFromBuffer(BoosterHandle handle, const void* buf, bst_ulong len) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  adopt_model(*b, load_model_buffer(buf, (size_t)len));
  API_END();
}

int XGBoosterSaveModel(BoosterHandle handle, const char* fname) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  if (fname == nullptr) throw OhxError("XGBoosterSaveModel: fname is NULL");
  if (!b->loaded) throw OhxError("XGBoosterSaveModel: the booster holds no model");
  save_model_file(b->forest, fname);
  API_END();
}

int XGBoosterSetParam(BoosterHandle handle, const char* name, const char* value) {
  API_BEGIN();
  if (name == nullptr || value == nullptr) throw OhxError("XGBoosterSetParam: NULL argument");
  const std::string n(name), v(value);
  if (n == "ohx_copy_engine") {                               // process-wide; the handle may be NULL
    if (v != "kernel" && v != "dma" && v != "auto") throw OhxError("ohx_copy_engine must be kernel, dma or auto");
    g_copy_engine.store(v == "kernel" ? kCopyKernel : (v == "dma" ? kCopyDma : kCopyAuto));
    return 0;
  }
  if (n == "ohx_register_host" && handle == nullptr) {       // process-wide: settable before any booster exists
    g_host_registry.on.store(atoi(value) != 0);
    if (atoi(value) == 0) g_host_registry.release_all();
    return 0;
  }
  BoosterObj* b = as_booster(handle);
  if (n == "ohx_kernel") {
    KernelKind named;
    if (v != "auto" && !kind_of_name(v, &named))
      throw OhxError("ohx_kernel must be one of auto, wide, packed1, packed2, packed4, super1 .. super4, ring");
    if (v != b->kernel_name) invalidate_device_state(*b);
    b->kernel_name = v;
  } else if (n == "ohx_top_levels") {
    int k = atoi(value);
    if (k < 1 || k > 30) throw OhxError("ohx_top_levels must be in 1..30");
    if (k != b->layout.top_levels) invalidate_device_state(*b);
    b->layout.top_levels = k;
  } else if (n == "ohx_line_slots") {
    int k = atoi(value);
    if (k < 0 || k > 1024 || (k & 1)) throw OhxError("ohx_line_slots must be even, 0..1024");
    if (k != b->layout.line_slots) invalidate_device_state(*b);
    b->layout.line_slots = k;
  } else if (n == "ohx_min_chunk") {
    int k = atoi(value);
    if (k < 2 || k > 1024) throw OhxError("ohx_min_chunk must be in 2..1024");
    if (k != b->layout.min_chunk) invalidate_device_state(*b);
    b->layout.min_chunk = k;
  } else if (n == "ohx_super_pack") {
    int k = atoi(value);
    if (k < kSuperPackNone || k > kSuperPackFamilies) throw OhxError("ohx_super_pack must be in 0..3");
    if (k != b->layout.super_pack) invalidate_device_state(*b);
    b->layout.super_pack = k;
  } else if (n == "ohx_launches_per_residency") {
    int k = atoi(value);
    if (k < 0 || k > 1000000) throw OhxError("ohx_launches_per_residency must be >= 0");
    b->tune.launches_per_residency = k;
  } else if (n == "ohx_brick") {
    // "bi,bj,bk": gridcells a wave takes along i, j, k (powers of two, product 64); "auto" = chosen per
    // call for the fewest idle lanes; "0,0,0" = 64 consecutive rows
    int e[3] = {-1, -1, -1}, lg[3] = {0, 0, 0};
    if (v == "auto") {
      b->tune.brick_li = b->tune.brick_lj = b->tune.brick_lk = -1;
    } else if (sscanf(value, "%d,%d,%d", &e[0], &e[1], &e[2]) != 3) {
      throw OhxError("ohx_brick must be \"bi,bj,bk\" or \"auto\"");
    } else if (e[0] == 0 && e[1] == 0 && e[2] == 0) {
      b->tune.brick_li = b->tune.brick_lj = b->tune.brick_lk = 0;
    } else {
      for (int q = 0; q < 3; ++q) {
        if (e[q] < 1 || e[q] > 64 || (e[q] & (e[q] - 1))) throw OhxError("ohx_brick extents must be powers of two");
        while ((1 << lg[q]) < e[q]) ++lg[q];
      }
      if (lg[0] + lg[1] + lg[2] != 6) throw OhxError("ohx_brick extents must multiply to 64");
      b->tune.brick_li = lg[0];
      b->tune.brick_lj = lg[1];
      b->tune.brick_lk = lg[2];
    }
  } else if (n == "ohx_brick_k_fastest") {
    b->tune.brick_k_fastest = atoi(value) != 0;
  } else if (n == "ohx_cluster") {
    // rows in no known order: "auto" groups them by tree-top decisions unless they look ordered; "on" / "off"
    if (v == "auto") b->tune.cluster = -1;
    else if (v == "on" || v == "1") b->tune.cluster = 1;
    else if (v == "off" || v == "0") b->tune.cluster = 0;
    else throw OhxError("ohx_cluster must be auto, on or off");
  } else if (n == "ohx_cluster_trees") {
    b->tune.cluster_trees = std::max(1, atoi(value));
  } else if (n == "ohx_cluster_zorder") {
    b->tune.cluster_zorder = atoi(value) != 0;
  } else if (n == "ohx_cluster_steps") {
    b->tune.cluster_steps = std::max(1, atoi(value));
  } else if (n == "ohx_lds_pad") {
    b->tune.lds_pad = atoi(value);
  } else if (n == "ohx_register_host") {
    // process-wide (the host form of OHXOHPostProcess has no booster): see HostRegistry
    g_host_registry.on.store(atoi(value) != 0);
    if (atoi(value) == 0) g_host_registry.release_all();
  } else if (n == "ohx_reserve_cus") {
    const int k = atoi(value);
    if (k < 0 || k > 128) throw OhxError("ohx_reserve_cus must be 0..128");
    b->tune.reserve_cus = k;
  } else if (n == "ohx_ring_rounds") {
    const int k = atoi(value);
    if (k < 0) throw OhxError("ohx_ring_rounds must be >= 0");
    b->tune.ring_rounds = k;
  } else if (n == "ohx_copy_blocks") {
    g_copy_blocks.store((uint32_t)std::max(0, atoi(value)));
  } else if (n == "ohx_run1_pieces") {
    const int k = atoi(value);
    if (k < 0 || k > 64) throw OhxError("ohx_run1_pieces must be 0 .. 64 (0 and 1: one piece)");
    b->tune.run1_pieces = k;
  } else if (n == "ohx_tree_split") {
    if (v == "auto") b->tune.tree_split = -1;
    else if (v == "off") b->tune.tree_split = 0;
    else {
      const int k = atoi(value);
      if (k < 2 || k > 10) throw OhxError("ohx_tree_split must be auto, off or 2..10");
      b->tune.tree_split = k;
    }
  } else if (n == "ohx_defer_missing") {
    if (v != "auto" && v != "on" && v != "off") throw OhxError("ohx_defer_missing must be auto, on or off");
    b->tune.defer_missing = v == "auto" ? -1 : (v == "on" ? 1 : 0);
  } else if (n == "ohx_prefetch") {
    b->tune.prefetch = atoi(value) != 0;
  } else if (n == "ohx_coop_rows") {
    b->tune.coop_rows = atoi(value) != 0;
  } else if (n == "ohx_xcd_remap") {
    b->tune.xcd_remap = atoi(value) != 0;
  } else if (n == "ohx_overlap_group") {
    const int k = atoi(value);
    if (k < 0) throw OhxError("ohx_overlap_group must be >= 0");
    b->tune.overlap_group = k;
    if (b->uploaded) {
      HIP_CHECK(hipSetDevice(b->dev.ordinal));
      ensure_train_stream(*b);
    }
  } else if (n == "ohx_tree_tops") {
    const std::string v = value;
    if (v != "auto" && v != "on" && v != "off") throw OhxError("ohx_tree_tops must be auto, on or off");
    b->tune.tree_tops = v == "auto" ? -1 : (v == "on" ? 1 : 0);
  } else if (n == "ohx_contribs_split") {
    const std::string v = value;
    if (v != "auto" && v != "off") throw OhxError("ohx_contribs_split must be auto or off");
    b->contribs_split = v == "auto";
  } else if (n == "ohx_cat_kernel") {
    // boosters with categorical splits: "direct" = margins by the direct kernel too (the same bits as the tile kernel's)
    if (v != "auto" && v != "direct") throw OhxError("ohx_cat_kernel must be auto or direct");
    b->cat_force_direct = v == "direct";
  } else if (n == "ohx_visits_kernel") {
    // visit counts: "lds" = a tree whose leaf histogram fits keeps it in LDS; "global" = one global add per distinct leaf
    // and wave for every tree.  The same integers; auto is global, the faster of the two where it was measured
    // (docs/16_visit_counts.md 16.4)
    if (v != "auto" && v != "global" && v != "lds") throw OhxError("ohx_visits_kernel must be auto, global or lds");
    b->visits_use_lds = v == "lds";
  } else if (n == "ohx_visits_lds_leaves") {
    // visit counts, "ohx_visits_kernel" = lds: the most leaves a tree may have to keep its histogram in LDS ("auto" or
    // 0 = what fits a CU)
    long k = 0;
    if (v != "auto") {
      char* end = nullptr;
      k = strtol(value, &end, 10);
      if (v.empty() || end == value || *end != '\0' || k < 0 || k > 0x7FFFFFFFl)
        throw OhxError("ohx_visits_lds_leaves must be auto or a whole number >= 0");
    }
    b->visits_lds_leaves = (uint32_t)k;
  } else if (n == "ohx_objective") {
    // boosting: what a row's (gradient, hessian) pair is made from (docs/26_objectives.md); on the handle, in no file
    if (v != "squarederror" && v != "pseudohuber" && v != "quantile")
      throw OhxError("ohx_objective must be squarederror, pseudohuber or quantile");
    b->grow_objective = v == "pseudohuber" ? kGrowObjPseudoHuber : v == "quantile" ? kGrowObjQuantile : kGrowObjSquared;
  } else if (n == "ohx_huber_slope") {
    char* end = nullptr;
    const float k = strtof(value, &end);
    if (v.empty() || end == value || *end != '\0' || !grow_slope_sound(k))
      throw OhxError("ohx_huber_slope must be a decimal number with 2^-10 <= slope <= 256");
    b->grow_slope = k;
  } else if (n == "ohx_quantile_alpha") {
    // boosting: alpha of the quantile objective and metric (docs/32_quantile_objective.md); on the handle, in no file
    char* end = nullptr;
    const float k = strtof(value, &end);
    if (v.empty() || end == value || *end != '\0' || !grow_alpha_sound(k))
      throw OhxError("ohx_quantile_alpha must be a decimal number with 2^-10 <= alpha <= 1 - 2^-10");
    b->grow_quantile_alpha = k;
  } else if (n == "ohx_reg_alpha" || n == "ohx_max_delta_step") {
    // boosting: CalcWeight / CalcGain's other two parameters (docs/27_regularisation_and_metrics.md); on the handle, in no file
    char* end = nullptr;
    const float k = strtof(value, &end);
    if (v.empty() || end == value || *end != '\0' || !grow_reg_sound(k))
      throw OhxError(n + " must be a finite decimal number >= 0");
    (n == "ohx_reg_alpha" ? b->grow_alpha : b->grow_max_delta_step) = k;
  } else if (n == "ohx_eval_metric") {
    if (v != "rmse" && v != "mae" && v != "pseudohuber" && v != "quantile")
      throw OhxError("ohx_eval_metric must be rmse, mae, pseudohuber or quantile");
    b->grow_metric = v == "mae"           ? kGrowMetricMae
                     : v == "pseudohuber" ? kGrowMetricPseudoHuber
                     : v == "quantile"    ? kGrowMetricQuantile
                                          : kGrowMetricRmse;
  } else if (n == "ohx_monotone_constraints") {
    // boosting: c_f of every feature (docs/28_monotone_constraints.md); on the handle, in no file
    b->grow_mono = parse_monotone_constraints(value);
  } else if (n == "ohx_interaction_constraints") {
    // boosting: the groups of features that may act together in a tree (docs/35_interaction_constraints.md); on the
    // handle, in no file
    b->grow_interact = parse_interaction_constraints(value);
  } else if (n == "ohx_colsample_bylevel" || n == "ohx_colsample_bynode") {
    // boosting: the fraction of a tree's features a level sees, and of a level's a node does
    // (docs/29_colsample_level_node.md); on the handle, in no file
    char* end = nullptr;
    const float k = strtof(value, &end);
    if (v.empty() || end == value || *end != '\0' || !(k > 0.0f && k <= 1.0f))
      throw OhxError(n + " must be a finite decimal number with 0 < v <= 1");
    (n == "ohx_colsample_bylevel" ? b->grow_bylevel : b->grow_bynode) = k;
  } else if (n == "ohx_grow_pairs") {
    // "on": squared error goes through the pair kernels too (the same bits); auto: only an objective that needs them
    if (v != "auto" && v != "on") throw OhxError("ohx_grow_pairs must be auto or on");
    b->grow_pairs_on = v == "on";
  } else if (n == "ohx_device") {
    int k = atoi(value);
    if (k != b->device_pref) {
      invalidate_device_state(*b);
      drop_leaf_walk(*b);              // the visit counts live on the device they were counted on
      b->grow.reset();
    }
    b->device_pref = k;
  }
  // any other name is an xgboost training/runtime parameter with no meaning here
  API_END();
}

int XGBoosterPredict(BoosterHandle handle, DMatrixHandle dmat, int option_mask, unsigned ntree_limit, int training,
                     bst_ulong* out_len, const float** out_result) {
  API_BEGIN();
  (void)training;
  BoosterObj* b = as_booster(handle);
  DMatrixObj* d = as_dmat(dmat);
  if (out_len == nullptr || out_result == nullptr) throw OhxError("XGBoosterPredict: NULL output argument");
  if (!b->loaded) throw OhxError("the booster holds no model: call XGBoosterLoadModel first");
  uint32_t t0, t1;
  tree_range(*b, ntree_limit, &t0, &t1);
  const size_t per_row = (option_mask == 16) ? (size_t)(t1 - t0) : 1;
  const size_t count = b->num_groups >= 2 ? group_predict_len(*b, d->nrow, option_mask, ntree_limit) : (size_t)d->nrow * per_row;
  ensure_uploaded(*b);
  b->d_pred.ensure(count);
  b->h_pred.ensure(count);
  if (d->owned == nullptr) order_behind_caller(b->dev.ordinal, b->s_exec);
  launch_predict_checked(*b, *d, option_mask, ntree_limit, b->d_pred.p, b->s_exec);
  if (count) HIP_CHECK(hipMemcpyAsync(b->h_pred.p, b->d_pred.p, count * sizeof(float), hipMemcpyDeviceToHost, b->s_exec));
  raise_flag_errors(*b, b->s_exec);              // waits for the stream: the predictions are in h_pred
  *out_len = count;
  *out_result = b->h_pred.p;
  API_END();
}

int OHXBoosterPredictDevice(BoosterHandle handle, DMatrixHandle dmat, int option_mask, unsigned ntree_limit,
                            float* d_out, void* stream) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  DMatrixObj* d = as_dmat(dmat);
  if (d_out == nullptr && d->nrow != 0) throw OhxError("OHXBoosterPredictDevice: d_out is NULL");
  d->used_async = true;
  launch_predict_checked(*b, *d, option_mask, ntree_limit, d_out, static_cast<hipStream_t>(stream));
  API_END();
}

int OHXBoosterPredictContribs(BoosterHandle handle, DMatrixHandle dmat, int approximate, unsigned ntree_limit,
                              bst_ulong* out_len, const float** out_result) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  refuse_categorical(*b, "OHXBoosterPredictContribs");
  ExplainCall q;
  q.name = "OHXBoosterPredictContribs";
  q.d = as_dmat(dmat);
  if (out_len == nullptr || out_result == nullptr) throw OhxError("OHXBoosterPredictContribs: NULL output argument");
  q.approximate = approximate;
  q.ntree_limit = ntree_limit;
  q.host_form = true;
  const ExplainResult r = explain(*b, q);
  *out_len = r.count;
  *out_result = r.host;
  API_END();
}

int OHXBoosterPredictContribsDevice(BoosterHandle handle, DMatrixHandle dmat, int approximate, unsigned ntree_limit,
                                    float* d_out, void* stream) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  refuse_categorical(*b, "OHXBoosterPredictContribsDevice");
  ExplainCall q;
  q.name = "OHXBoosterPredictContribsDevice";
  q.d = as_dmat(dmat);
  q.approximate = approximate;
  q.ntree_limit = ntree_limit;
  q.d_out = d_out;
  q.stream = static_cast<hipStream_t>(stream);
  explain(*b, q);
  q.d->used_async = true;
  API_END();
}

int OHXBoosterPredictInteractions(BoosterHandle handle, DMatrixHandle dmat, int approximate, unsigned ntree_limit,
                                  bst_ulong* out_len, const float** out_result) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  refuse_categorical(*b, "OHXBoosterPredictInteractions");
  ExplainCall q;
  q.name = "OHXBoosterPredictInteractions";
  q.interactions = true;
  q.d = as_dmat(dmat);
  if (out_len == nullptr || out_result == nullptr)
    throw OhxError("OHXBoosterPredictInteractions: NULL output argument");
  q.approximate = approximate;
  q.ntree_limit = ntree_limit;
  q.host_form = true;
  const ExplainResult r = explain(*b, q);
  *out_len = r.count;
  *out_result = r.host;
  API_END();
}

int OHXBoosterPredictInteractionsDevice(BoosterHandle handle, DMatrixHandle dmat, int approximate,
                                        unsigned ntree_limit, float* d_out, void* stream) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  refuse_categorical(*b, "OHXBoosterPredictInteractionsDevice");
  ExplainCall q;
  q.name = "OHXBoosterPredictInteractionsDevice";
  q.interactions = true;
  q.d = as_dmat(dmat);
  q.approximate = approximate;
  q.ntree_limit = ntree_limit;
  q.d_out = d_out;
  q.stream = static_cast<hipStream_t>(stream);
  explain(*b, q);
  q.d->used_async = true;
  API_END();
}

int OHXBoosterCountVisits(BoosterHandle handle, DMatrixHandle dmat) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  count_visits(*b, dmat, true, nullptr, "OHXBoosterCountVisits");
  API_END();
}

int OHXBoosterCountVisitsDevice(BoosterHandle handle, DMatrixHandle dmat, void* stream) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  count_visits(*b, dmat, false, static_cast<hipStream_t>(stream), "OHXBoosterCountVisitsDevice");
  API_END();
}

int OHXBoosterGetVisitCounts(BoosterHandle handle, void* stream, bst_ulong* ntree, const bst_ulong** tree_offsets,
                             const uint64_t** counts, uint64_t* rows_seen) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  VisitState& v = visits_begin(*b, "OHXBoosterGetVisitCounts");
  if (ntree == nullptr || tree_offsets == nullptr || counts == nullptr || rows_seen == nullptr)
    throw OhxError("OHXBoosterGetVisitCounts: NULL output argument");
  read_visit_counts(*b, v, static_cast<hipStream_t>(stream));
  static_assert(sizeof(bst_ulong) == sizeof(uint64_t), "tree_offsets are handed out as bst_ulong");
  *ntree = b->forest.trees.size();
  *tree_offsets = reinterpret_cast<const bst_ulong*>(b->leaf_walk->vf.tree_offsets.data());
  *counts = v.node_counts.data();
  *rows_seen = v.rows_seen;
  API_END();
}

int OHXBoosterResetVisitCounts(BoosterHandle handle) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  VisitState& v = visits_begin(*b, "OHXBoosterResetVisitCounts");
  if (v.device >= 0) {
    // behind every count, whatever stream it was enqueued on
    HIP_CHECK(hipSetDevice(v.device));
    HIP_CHECK(hipDeviceSynchronize());
    hipStream_t s = lib_streams(v.device).exec;
    HIP_CHECK(hipMemsetAsync(v.d_counts.p, 0, v.d_counts.n * sizeof(unsigned long long), s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  std::fill(v.node_counts.begin(), v.node_counts.end(), 0);
  v.rows_seen = 0;
  API_END();
}

int OHXBoosterRefreshCover(BoosterHandle handle, void* stream, float prior_weight) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  VisitState& v = visits_begin(*b, "OHXBoosterRefreshCover");
  if (!(std::isfinite(prior_weight) && prior_weight >= 0.0f))
    throw OhxError("OHXBoosterRefreshCover: prior_weight must be finite and >= 0");
  if (v.rows_seen == 0)
    throw OhxError("OHXBoosterRefreshCover: no row has been counted yet (OHXBoosterCountVisits); the covers are unchanged");
  read_visit_counts(*b, v, static_cast<hipStream_t>(stream));
  // all or nothing: every new cover is computed (and every split's judged) before the first one is stored
  std::vector<std::vector<float>> covers = refreshed_covers(b->forest, b->leaf_walk->vf, v.node_counts.data(), prior_weight);
  for (size_t t = 0; t < covers.size(); ++t) b->forest.trees[t].sum_hess = std::move(covers[t]);
  // the contributions' tables hold the old covers: dropped exactly as a model load drops them, rebuilt at the next call
  b->contribs.reset();
  API_END();
}

int OHXBoosterRefitLeaves(BoosterHandle handle, DMatrixHandle dmat, const float* labels, bst_ulong nlabel, float eta,
                          float lambda, int unvisited, bst_ulong* leaves_refit) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  refit_leaves(*b, dmat, labels, nlabel, eta, lambda, unvisited, leaves_refit, true, nullptr, "OHXBoosterRefitLeaves");
  API_END();
}

int OHXBoosterRefitLeavesDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels, bst_ulong nlabel,
                                float eta, float lambda, int unvisited, bst_ulong* leaves_refit, void* stream) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  refit_leaves(*b, dmat, d_labels, nlabel, eta, lambda, unvisited, leaves_refit, false, static_cast<hipStream_t>(stream),
               "OHXBoosterRefitLeavesDevice");
  API_END();
}

int OHXBoosterBoostTrees(BoosterHandle handle, DMatrixHandle dmat, const float* labels, bst_ulong nlabel,
                         const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth, float eta,
                         float lambda, float gamma, bst_ulong min_child_rows, bst_ulong* nodes_added) {
  API_BEGIN();
  BoostCall c = boost_call("OHXBoosterBoostTrees", true, nullptr, dmat, labels, nlabel, cut_ptr, cut_values, rounds, max_depth,
                           eta, lambda, gamma, nodes_added);
  c.min_child_rows = min_child_rows;
  boost_trees(*as_booster(handle), c);
  API_END();
}

int OHXBoosterBoostTreesDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels, bst_ulong nlabel,
                               const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth, float eta,
                               float lambda, float gamma, bst_ulong min_child_rows, bst_ulong* nodes_added, void* stream) {
  API_BEGIN();
  BoostCall c = boost_call("OHXBoosterBoostTreesDevice", false, stream, dmat, d_labels, nlabel, cut_ptr, cut_values, rounds,
                           max_depth, eta, lambda, gamma, nodes_added);
  c.min_child_rows = min_child_rows;
  boost_trees(*as_booster(handle), c);
  API_END();
}

int OHXBoosterBoostTreesEval(BoosterHandle handle, DMatrixHandle dmat, const float* labels, bst_ulong nlabel,
                             DMatrixHandle eval_dmat, const float* eval_labels, bst_ulong eval_nlabel,
                             const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth, float eta,
                             float lambda, float gamma, bst_ulong min_child_rows, int patience, double* train_rmse,
                             double* eval_rmse, int* rounds_run, int* best_round, bst_ulong* nodes_added) {
  API_BEGIN();
  BoostCall c = boost_call("OHXBoosterBoostTreesEval", true, nullptr, dmat, labels, nlabel, cut_ptr, cut_values, rounds,
                           max_depth, eta, lambda, gamma, nodes_added);
  c.min_child_rows = min_child_rows;
  c.eval = boost_eval(eval_dmat, eval_labels, eval_nlabel, patience, train_rmse, eval_rmse, rounds_run, best_round);
  boost_trees(*as_booster(handle), c);
  API_END();
}

int OHXBoosterBoostTreesEvalDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels, bst_ulong nlabel,
                                   DMatrixHandle eval_dmat, const float* d_eval_labels, bst_ulong eval_nlabel,
                                   const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth, float eta,
                                   float lambda, float gamma, bst_ulong min_child_rows, int patience, double* train_rmse,
                                   double* eval_rmse, int* rounds_run, int* best_round, bst_ulong* nodes_added,
                                   void* stream) {
  API_BEGIN();
  BoostCall c = boost_call("OHXBoosterBoostTreesEvalDevice", false, stream, dmat, d_labels, nlabel, cut_ptr, cut_values, rounds,
                           max_depth, eta, lambda, gamma, nodes_added);
  c.min_child_rows = min_child_rows;
  c.eval = boost_eval(eval_dmat, d_eval_labels, eval_nlabel, patience, train_rmse, eval_rmse, rounds_run, best_round);
  boost_trees(*as_booster(handle), c);
  API_END();
}

int OHXBoosterBoostTreesWeighted(BoosterHandle handle, DMatrixHandle dmat, const float* labels, const float* weights,
                                 bst_ulong nlabel, DMatrixHandle eval_dmat, const float* eval_labels,
                                 const float* eval_weights, bst_ulong eval_nlabel, const bst_ulong* cut_ptr,
                                 const float* cut_values, int rounds, int max_depth, float eta, float lambda, float gamma,
                                 float min_child_weight, int patience, double* train_rmse, double* eval_rmse,
                                 int* rounds_run, int* best_round, bst_ulong* nodes_added) {
  API_BEGIN();
  BoostCall c = boost_call("OHXBoosterBoostTreesWeighted", true, nullptr, dmat, labels, nlabel, cut_ptr, cut_values, rounds,
                           max_depth, eta, lambda, gamma, nodes_added);
  c.eval = boost_eval(eval_dmat, eval_labels, eval_nlabel, patience, train_rmse, eval_rmse, rounds_run, best_round);
  c.weights = boost_weights(weights, eval_weights, min_child_weight);
  boost_trees(*as_booster(handle), c);
  API_END();
}

int OHXBoosterBoostTreesWeightedDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels,
                                       const float* d_weights, bst_ulong nlabel, DMatrixHandle eval_dmat,
                                       const float* d_eval_labels, const float* d_eval_weights, bst_ulong eval_nlabel,
                                       const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth,
                                       float eta, float lambda, float gamma, float min_child_weight, int patience,
                                       double* train_rmse, double* eval_rmse, int* rounds_run, int* best_round,
                                       bst_ulong* nodes_added, void* stream) {
  API_BEGIN();
  BoostCall c = boost_call("OHXBoosterBoostTreesWeightedDevice", false, stream, dmat, d_labels, nlabel, cut_ptr, cut_values,
                           rounds, max_depth, eta, lambda, gamma, nodes_added);
  c.eval = boost_eval(eval_dmat, d_eval_labels, eval_nlabel, patience, train_rmse, eval_rmse, rounds_run, best_round);
  c.weights = boost_weights(d_weights, d_eval_weights, min_child_weight);
  boost_trees(*as_booster(handle), c);
  API_END();
}

int OHXBoosterBoostTreesSampled(BoosterHandle handle, DMatrixHandle dmat, const float* labels, const float* weights,
                                bst_ulong nlabel, DMatrixHandle eval_dmat, const float* eval_labels,
                                const float* eval_weights, bst_ulong eval_nlabel, const bst_ulong* cut_ptr,
                                const float* cut_values, int rounds, int max_depth, float eta, float lambda, float gamma,
                                float min_child_weight, float subsample, float colsample_bytree, uint64_t seed, int patience,
                                double* train_rmse, double* eval_rmse, int* rounds_run, int* best_round,
                                bst_ulong* nodes_added) {
  API_BEGIN();
  BoostCall c = boost_call("OHXBoosterBoostTreesSampled", true, nullptr, dmat, labels, nlabel, cut_ptr, cut_values, rounds,
                           max_depth, eta, lambda, gamma, nodes_added);
  c.eval = boost_eval(eval_dmat, eval_labels, eval_nlabel, patience, train_rmse, eval_rmse, rounds_run, best_round);
  c.weights = boost_weights(weights, eval_weights, min_child_weight);
  c.sampling = {true, subsample, colsample_bytree, seed};
  boost_trees(*as_booster(handle), c);
  API_END();
}

int OHXBoosterBoostTreesSampledDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels,
                                      const float* d_weights, bst_ulong nlabel, DMatrixHandle eval_dmat,
                                      const float* d_eval_labels, const float* d_eval_weights, bst_ulong eval_nlabel,
                                      const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth,
                                      float eta, float lambda, float gamma, float min_child_weight, float subsample,
                                      float colsample_bytree, uint64_t seed, int patience, double* train_rmse,
                                      double* eval_rmse, int* rounds_run, int* best_round, bst_ulong* nodes_added,
                                      void* stream) {
  API_BEGIN();
  BoostCall c = boost_call("OHXBoosterBoostTreesSampledDevice", false, stream, dmat, d_labels, nlabel, cut_ptr, cut_values,
                           rounds, max_depth, eta, lambda, gamma, nodes_added);
  c.eval = boost_eval(eval_dmat, d_eval_labels, eval_nlabel, patience, train_rmse, eval_rmse, rounds_run, best_round);
  c.weights = boost_weights(d_weights, d_eval_weights, min_child_weight);
  c.sampling = {true, subsample, colsample_bytree, seed};
  boost_trees(*as_booster(handle), c);
  API_END();
}

int OHXBoosterBoostTreesDeep(BoosterHandle handle, DMatrixHandle dmat, const float* labels, const float* weights,
                             bst_ulong nlabel, DMatrixHandle eval_dmat, const float* eval_labels, const float* eval_weights,
                             bst_ulong eval_nlabel, const bst_ulong* cut_ptr, const float* cut_values, int rounds,
                             int max_depth, float eta, float lambda, float gamma, float min_child_weight, int patience,
                             double* train_rmse, double* eval_rmse, int* rounds_run, int* best_round,
                             bst_ulong* nodes_added) {
  API_BEGIN();
  BoostCall c = boost_call("OHXBoosterBoostTreesDeep", true, nullptr, dmat, labels, nlabel, cut_ptr, cut_values, rounds,
                           max_depth, eta, lambda, gamma, nodes_added);
  c.eval = boost_eval(eval_dmat, eval_labels, eval_nlabel, patience, train_rmse, eval_rmse, rounds_run, best_round);
  c.weights = boost_weights(weights, eval_weights, min_child_weight);
  c.deep = true;
  boost_trees(*as_booster(handle), c);
  API_END();
}

int OHXBoosterBoostTreesDeepDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels, const float* d_weights,
                                   bst_ulong nlabel, DMatrixHandle eval_dmat, const float* d_eval_labels,
                                   const float* d_eval_weights, bst_ulong eval_nlabel, const bst_ulong* cut_ptr,
                                   const float* cut_values, int rounds, int max_depth, float eta, float lambda, float gamma,
                                   float min_child_weight, int patience, double* train_rmse, double* eval_rmse,
                                   int* rounds_run, int* best_round, bst_ulong* nodes_added, void* stream) {
  API_BEGIN();
  BoostCall c = boost_call("OHXBoosterBoostTreesDeepDevice", false, stream, dmat, d_labels, nlabel, cut_ptr, cut_values,
                           rounds, max_depth, eta, lambda, gamma, nodes_added);
  c.eval = boost_eval(eval_dmat, d_eval_labels, eval_nlabel, patience, train_rmse, eval_rmse, rounds_run, best_round);
  c.weights = boost_weights(d_weights, d_eval_weights, min_child_weight);
  c.deep = true;
  boost_trees(*as_booster(handle), c);
  API_END();
}

int OHXBoosterBoostTreesDeepSampled(BoosterHandle handle, DMatrixHandle dmat, const float* labels, const float* weights,
                                    bst_ulong nlabel, DMatrixHandle eval_dmat, const float* eval_labels,
                                    const float* eval_weights, bst_ulong eval_nlabel, const bst_ulong* cut_ptr,
                                    const float* cut_values, int rounds, int max_depth, float eta, float lambda, float gamma,
                                    float min_child_weight, float subsample, float colsample_bytree, uint64_t seed,
                                    int patience, double* train_rmse, double* eval_rmse, int* rounds_run, int* best_round,
                                    bst_ulong* nodes_added) {
  API_BEGIN();
  BoostCall c = boost_call("OHXBoosterBoostTreesDeepSampled", true, nullptr, dmat, labels, nlabel, cut_ptr, cut_values, rounds,
                           max_depth, eta, lambda, gamma, nodes_added);
  c.eval = boost_eval(eval_dmat, eval_labels, eval_nlabel, patience, train_rmse, eval_rmse, rounds_run, best_round);
  c.weights = boost_weights(weights, eval_weights, min_child_weight);
  c.sampling = {true, subsample, colsample_bytree, seed};
  c.deep = true;
  boost_trees(*as_booster(handle), c);
  API_END();
}

int OHXBoosterBoostTreesDeepSampledDevice(BoosterHandle handle, DMatrixHandle dmat, const float* d_labels,
                                          const float* d_weights, bst_ulong nlabel, DMatrixHandle eval_dmat,
                                          const float* d_eval_labels, const float* d_eval_weights, bst_ulong eval_nlabel,
                                          const bst_ulong* cut_ptr, const float* cut_values, int rounds, int max_depth,
                                          float eta, float lambda, float gamma, float min_child_weight, float subsample,
                                          float colsample_bytree, uint64_t seed, int patience, double* train_rmse,
                                          double* eval_rmse, int* rounds_run, int* best_round, bst_ulong* nodes_added,
                                          void* stream) {
  API_BEGIN();
  BoostCall c = boost_call("OHXBoosterBoostTreesDeepSampledDevice", false, stream, dmat, d_labels, nlabel, cut_ptr, cut_values,
                           rounds, max_depth, eta, lambda, gamma, nodes_added);
  c.eval = boost_eval(eval_dmat, d_eval_labels, eval_nlabel, patience, train_rmse, eval_rmse, rounds_run, best_round);
  c.weights = boost_weights(d_weights, d_eval_weights, min_child_weight);
  c.sampling = {true, subsample, colsample_bytree, seed};
  c.deep = true;
  boost_trees(*as_booster(handle), c);
  API_END();
}

int OHXQuantileCuts(const float* data, bst_ulong nrow, bst_ulong ncol, float missing, int max_bins, bst_ulong* cut_ptr,
                    float* cut_values, bst_ulong cap, bst_ulong* needed) {
  API_BEGIN();
  if (cut_ptr == nullptr || needed == nullptr) throw OhxError("OHXQuantileCuts: NULL output argument");
  if (data == nullptr && nrow * ncol != 0) throw OhxError("OHXQuantileCuts: data is NULL");
  if (cut_values == nullptr && cap != 0) throw OhxError("OHXQuantileCuts: cut_values is NULL");
  if (max_bins < 2 || max_bins > 255) throw OhxError("OHXQuantileCuts: max_bins must be in 2..255");
  static_assert(sizeof(bst_ulong) == sizeof(uint64_t), "bst_ulong is uint64");
  *needed = quantile_cuts(data, nrow, ncol, missing, max_bins, reinterpret_cast<uint64_t*>(cut_ptr), cut_values, cap);
  if (*needed > cap)
    throw OhxError("OHXQuantileCuts: " + std::to_string(*needed) + " cut values are needed and cut_values holds " +
                   std::to_string(cap));
  API_END();
}

int OHXDMatrixQuantileCuts(DMatrixHandle dmat, bst_ulong row_step, int max_bins, bst_ulong* cut_ptr, float* cut_values,
                           bst_ulong cap, bst_ulong* needed, void* stream) {
  API_BEGIN();
  dmatrix_quantile_cuts(dmat, row_step, max_bins, cut_ptr, cut_values, cap, needed, static_cast<hipStream_t>(stream));
  API_END();
}

int OHXBoosterCheck(BoosterHandle handle, void* stream) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  ensure_uploaded(*b);
  raise_flag_errors(*b, static_cast<hipStream_t>(stream));
  API_END();
}

// `fields`: the device form's, checked and taken here; the host form (nullptr) checks its own as it stages them
static void fields_common(BoosterObj& b, FieldsArgs& a, const float* const fields[], const int32_t is2d[], int nfield,
                          int pl_feature, int im, int jm, int km, int k1, int k2, float missing, int apply_pow10,
                          float ohscale) {
  check_fields_shape(b, nfield, im, jm, km, k1, k2);
  if (!objective_is_identity(b.forest.objective))
    throw OhxError("objective '" + b.forest.objective + "' is not supported by predict_fields");
  fields_preamble(a, fields, is2d, nfield, pl_feature);
  for (int f = 0; fields != nullptr && f < nfield; ++f) a.field[f] = fields[f];
  a.im = im;
  a.jm = jm;
  a.km = km;
  a.k1 = k1 - 1;
  a.k2 = k2 - 1;
  a.missing = missing;
  tree_range(b, 0, &a.tree_begin, &a.tree_end);
  a.apply_pow10 = apply_pow10;
  a.scale = ohscale;
  a.flags = b.d_flags.p;
}

int OHXBoosterPredictFieldsDevice(BoosterHandle handle, const float* const d_fields[], const int32_t is2d[],
                                  int nfield, int pl_feature, int im, int jm, int km, int k1, int k2, float missing,
                                  int apply_pow10, float ohscale, float* d_oh_ml, float* d_margin, void* stream) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  refuse_groups(*b, "OHXBoosterPredictFieldsDevice");
  refuse_categorical(*b, "OHXBoosterPredictFieldsDevice");
  if (d_fields == nullptr || is2d == nullptr || d_oh_ml == nullptr) throw OhxError("predict_fields: NULL argument");
  ensure_uploaded(*b);
  FieldsArgs a{};
  fields_common(*b, a, d_fields, is2d, nfield, pl_feature, im, jm, km, k1, k2, missing, apply_pow10, ohscale);
  a.out = d_oh_ml;
  a.margin_out = d_margin;
  if (pick_kernel(*b) == KernelKind::Wide) ensure_wide(*b);
  if (a.k2 >= a.k1) {
    const uint64_t nrow = (uint64_t)im * (uint64_t)jm * (uint64_t)(a.k2 - a.k1 + 1);
    hipStream_t s = static_cast<hipStream_t>(stream);
    walk_with_buffers(*b, nrow, a.tree_end - a.tree_begin, b->tune, im, jm, 0, true, nfield == 27, s, [&](const LaunchTuning& tune) {
      return launch_predict_fields(pick_kernel(*b), device_forest(*b), a, b->dev.num_cus, s, tune);
    });
  }
  API_END();
}

int OHXBoosterPredictFields(BoosterHandle handle, const float* const fields[], const int32_t is2d[], int nfield,
                            int pl_feature, int im, int jm, int km, int k1, int k2, float missing, int apply_pow10,
                            float ohscale, float* oh_ml, float* margin) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  refuse_groups(*b, "OHXBoosterPredictFields");
  refuse_categorical(*b, "OHXBoosterPredictFields");
  if (fields == nullptr || is2d == nullptr || oh_ml == nullptr) throw OhxError("predict_fields: NULL argument");
  ensure_uploaded(*b);
  FieldsArgs a{};
  fields_common(*b, a, nullptr, is2d, nfield, pl_feature, im, jm, km, k1, k2, missing, apply_pow10, ohscale);
  if (a.k2 < a.k1) return 0;
  const size_t plane = (size_t)im * (size_t)jm;
  const size_t nlev = (size_t)(a.k2 - a.k1 + 1);
  const size_t nrow = plane * nlev;
  if (b->d_stage.size() < (size_t)nfield) b->d_stage.resize((size_t)nfield);
  // Only the slab k1..k2 of each 3-D field crosses PCIe, and it crosses in pieces of whole
  // levels: while piece c is being walked on the compute stream, piece c+1 is already on its
  // way over PCIe on the copy stream (a step is PCIe-bound: 756 MB in, 28 MB out for a
  // C360/8 sub-domain, against ~6 ms of kernels).
  // pieces of at least two residencies of rows (the launch granule), at most 8 pieces
  const size_t min_rows = (size_t)64 * 256 * 20 * 2;
  size_t lev_per_piece = (min_rows + plane - 1) / plane;
  if (lev_per_piece * 8 < nlev) lev_per_piece = (nlev + 7) / 8;
  if (lev_per_piece < 1) lev_per_piece = 1;
  // A rank-sized block is ONE piece, and with the caller's arrays registered its 27 fields cross in one copy launch
  // (HostMover) instead of 27 copies at 27 fixed prices: a 48 x 24 x 72 block 0.55 -> 0.33 ms, 96 x 48 x 72 1.26 -> 1.03
  // (profiles/r04_sweeps.txt; the reference's five calls: 0.35 and 1.02)
  const bool registered = g_host_registry.on.load(std::memory_order_relaxed);
  const bool one_launch = registered && lev_per_piece >= nlev && nfield <= (int)kCopyListMax &&
                          ((size_t)nfield * nrow + nrow * 2) * sizeof(float) <= HostMover::kKernelBytesMax;
  HostMover in(b->s_exec, true);
  for (int f = 0; f < nfield; ++f) {
    if (fields[f] == nullptr) throw OhxError("predict_fields: field " + std::to_string(f) + " is NULL");
    b->d_stage[(size_t)f].ensure(is2d[f] ? plane : nrow);
    a.field[f] = b->d_stage[(size_t)f].p;
    if (one_launch) {
      if (is2d[f]) in.add(b->d_stage[(size_t)f].p, fields[f], plane);
      else in.add_slice(b->d_stage[(size_t)f].p, fields[f], plane * (size_t)km, plane * (size_t)a.k1, nrow);
    } else if (is2d[f]) {
      upload_host_array(b->d_stage[(size_t)f].p, fields[f], plane, b->s_copy);
    } else if (registered) {
      (void)g_host_registry.want(fields[f], plane * (size_t)km * sizeof(float));       // the whole field once, not per piece
    }
  }
  if (one_launch) in.go();
  a.src_k0 = a.k1;
  a.out_k0 = a.k1;
  b->d_stage_out.ensure(nrow);
  a.out = b->d_stage_out.p;
  if (margin) {
    b->d_stage_margin.ensure(nrow);
    a.margin_out = b->d_stage_margin.p;
  }
  if (pick_kernel(*b) == KernelKind::Wide) ensure_wide(*b);
  const float* margin_base = a.margin_out;
  std::vector<hipEvent_t> events;
  for (size_t l0 = 0; l0 < nlev; l0 += lev_per_piece) {
    const size_t l1 = std::min(nlev, l0 + lev_per_piece);
    for (int f = 0; f < nfield; ++f) {
      if (is2d[f] || one_launch) continue;
      const float* src = fields[f] + plane * ((size_t)a.k1 + l0);
      HIP_CHECK(hipMemcpyAsync(b->d_stage[(size_t)f].p + plane * l0, src, plane * (l1 - l0) * sizeof(float),
                               hipMemcpyHostToDevice, b->s_copy));
    }
    if (!one_launch) {           // (one launch: the list went to the kernels' own stream, in front of them)
      hipEvent_t ev;
      HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      events.push_back(ev);
      HIP_CHECK(hipEventRecord(ev, b->s_copy));
      HIP_CHECK(hipStreamWaitEvent(b->s_exec, ev, 0));
    }
    FieldsArgs piece = a;
    piece.k1 = a.k1 + (int)l0;
    piece.k2 = a.k1 + (int)l1 - 1;
    // rows of this piece start at plane * l0 of the slab-ordered margin buffer
    piece.margin_out = margin_base ? const_cast<float*>(margin_base) + plane * l0 : nullptr;
    walk_with_buffers(*b, plane * (l1 - l0), piece.tree_end - piece.tree_begin, b->tune, im, jm, 0, true, nfield == 27, b->s_exec,
                      [&](const LaunchTuning& tune) {
                        return launch_predict_fields(pick_kernel(*b), device_forest(*b), piece, b->dev.num_cus, b->s_exec, tune);
                      });
  }
  if (one_launch) {
    HostMover back(b->s_exec, false);
    back.add_slice(b->d_stage_out.p, oh_ml, plane * (size_t)km, plane * (size_t)a.k1, nrow);
    if (margin) back.add(margin, b->d_stage_margin.p, nrow);
    back.go();
  } else {
    if (registered) {
      (void)g_host_registry.want(oh_ml, plane * (size_t)km * sizeof(float));
      if (margin) (void)g_host_registry.want(margin, nrow * sizeof(float));
    }
    HIP_CHECK(hipMemcpyAsync(oh_ml + plane * (size_t)a.k1, b->d_stage_out.p, nrow * sizeof(float), hipMemcpyDeviceToHost,
                             b->s_exec));
    if (margin)
      HIP_CHECK(hipMemcpyAsync(margin, b->d_stage_margin.p, nrow * sizeof(float), hipMemcpyDeviceToHost, b->s_exec));
  }
  HIP_CHECK(hipStreamSynchronize(b->s_exec));
  for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
  raise_flag_errors(*b, b->s_exec);
  API_END();
}

// Contributions from the fields: the explanation call (explain, above) with the fields as its source.
int OHXBoosterPredictContribsFields(BoosterHandle handle, const float* const fields[], const int32_t is2d[],
                                    int nfield, int pl_feature, int im, int jm, int km, int k1, int k2, float missing,
                                    int approximate, unsigned ntree_limit, float* const out[]) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  refuse_groups(*b, "OHXBoosterPredictContribsFields");
  refuse_categorical(*b, "OHXBoosterPredictContribsFields");
  const FieldsSource fs{fields, is2d, nfield, pl_feature, im, jm, km, k1, k2, missing, out};
  ExplainCall q;
  q.name = "OHXBoosterPredictContribsFields";
  q.fs = &fs;
  q.approximate = approximate;
  q.ntree_limit = ntree_limit;
  q.host_form = true;
  explain(*b, q);
  API_END();
}

int OHXBoosterPredictContribsFieldsDevice(BoosterHandle handle, const float* const d_fields[], const int32_t is2d[],
                                          int nfield, int pl_feature, int im, int jm, int km, int k1, int k2,
                                          float missing, int approximate, unsigned ntree_limit, float* const d_out[],
                                          void* stream) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  refuse_groups(*b, "OHXBoosterPredictContribsFieldsDevice");
  refuse_categorical(*b, "OHXBoosterPredictContribsFieldsDevice");
  const FieldsSource fs{d_fields, is2d, nfield, pl_feature, im, jm, km, k1, k2, missing, d_out};
  ExplainCall q;
  q.name = "OHXBoosterPredictContribsFieldsDevice";
  q.fs = &fs;
  q.approximate = approximate;
  q.ntree_limit = ntree_limit;
  q.stream = static_cast<hipStream_t>(stream);
  explain(*b, q);
  API_END();
}

// ---- selected gridcells (include/ohxgb.h part 2b; cells.hip) ----
//
// No booster: the device forms enqueue on the caller's stream with the current device, the host forms stage through
// buffers of their own call on the library's stream.  The ordered passes (selection, scatter) keep one number per
// block in a table: the device forms' is one per (device, stream), made at the first call on that stream and kept for
// the life of the process - calls on one stream run one after the other, so they may share it - and both launches of
// a call are enqueued under the mutex, so two threads on one stream cannot interleave theirs.
extern "C++" {
namespace {
struct CellsTables {
  std::mutex mu;
  std::map<std::pair<int, hipStream_t>, uint64_t*> by_stream;
};
static CellsTables g_cells_tables;

// with g_cells_tables.mu held
uint64_t* cells_table(int device, hipStream_t stream) {
  uint64_t*& t = g_cells_tables.by_stream[{device, stream}];
  if (t == nullptr) {
    if (stream_capturing(stream))
      refuse_in_capture("allocate the per-block table of a selection or a scatter",
                        "make one plain call on this stream first, then capture");
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t), kCellsMaxBlocks * sizeof(uint64_t)));
  }
  return t;
}

SelectCellsArgs select_args(int im, int jm, int km, int i1, int i2, int j1, int j2, int k1, int k2, const float* a,
                            int a_is2d, const float* b, int b_is2d, float b0, const int64_t* cells, int64_t cap,
                            const int64_t* count) {
  check_grid_positive(im, jm, km);
  if (i1 < 1 || i2 > im || i2 < i1 - 1 || j1 < 1 || j2 > jm || j2 < j1 - 1 || k1 < 1 || k2 > km || k2 < k1 - 1)
    throw OhxError("select_cells: need 1 <= i1, i2 <= im, i2 >= i1 - 1, and the same for j and k");
  if (cap < 0) throw OhxError("select_cells: cap must not be negative");
  if (count == nullptr || (cells == nullptr && cap > 0)) throw OhxError("select_cells: NULL argument");
  SelectCellsArgs s;
  s.im = im;
  s.jm = jm;
  s.i0 = i1 - 1;
  s.j0 = j1 - 1;
  s.k0 = k1 - 1;
  s.wi = i2 - i1 + 1;
  s.wj = j2 - j1 + 1;
  s.wk = k2 - k1 + 1;
  s.a = a;
  s.b = a != nullptr ? b : nullptr;
  s.a_is2d = a_is2d != 0;
  s.b_is2d = b_is2d != 0;
  s.b0 = b0;
  s.cap = cap;
  return s;
}

GatherCellsArgs gather_args(const float* const fields[], const int32_t is2d[], int nfield, int pl_feature, int im,
                            int jm, int km, const int64_t* cells, int64_t ncell, const float* rows) {
  if (nfield < 1 || nfield > (int)kCellsMaxFields) throw OhxError("gather_cells: nfield must be 1..32");
  check_grid_positive(im, jm, km);
  if (ncell < 0) throw OhxError("gather_cells: ncell must not be negative");
  if (fields == nullptr || is2d == nullptr || (ncell > 0 && (cells == nullptr || rows == nullptr)))
    throw OhxError("predict_fields: NULL argument");
  GatherCellsArgs g{};
  fields_preamble(g, fields, is2d, nfield, pl_feature);
  for (int f = 0; f < nfield; ++f) g.field[f] = fields[f];
  g.plane = (int64_t)im * jm;
  g.ncells_total = g.plane * km;
  return g;
}

void scatter_check(const float* values, int64_t stride, int64_t col, const int64_t* cells, int64_t ncell,
                   const float* out3d, int im, int jm, int km) {
  check_grid_positive(im, jm, km);
  if (ncell < 0) throw OhxError("scatter_cells: ncell must not be negative");
  if (stride < 1 || col < 0 || col >= stride) throw OhxError("scatter_cells: need stride >= 1 and 0 <= col < stride");
  if (out3d == nullptr || (ncell > 0 && (values == nullptr || cells == nullptr)))
    throw OhxError("scatter_cells: NULL argument");
}

// the levels (0-based, inclusive) the in-range entries of a host list touch; false when there is none
bool cells_level_range(const int64_t* cells, int64_t ncell, int64_t plane, int64_t total, int64_t* lev0, int64_t* lev1) {
  int64_t lo = total, hi = -1;
  for (int64_t n = 0; n < ncell; ++n) {
    const int64_t c = cells[n];
    if (c < 0 || c >= total) continue;
    lo = std::min(lo, c);
    hi = std::max(hi, c);
  }
  if (hi < 0) return false;
  *lev0 = lo / plane;
  *lev1 = hi / plane;
  return true;
}

// a device pointer moved back by `off` floats: what the kernels index with whole-block cell indices when only a slab
// from element `off` on is staged (nothing in front of the slab is ever addressed)
float* slab_base(float* staged, int64_t off) {
  return reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(staged) - (uintptr_t)off * sizeof(float));
}
}  // namespace
}  // extern "C++"

int OHXSelectCellsDevice(int im, int jm, int km, int i1, int i2, int j1, int j2, int k1, int k2, const float* d_a,
                         int a_is2d, const float* d_b, int b_is2d, float b0, int64_t* d_cells, int64_t cap,
                         int64_t* d_count, uint32_t* d_status, void* stream) {
  API_BEGIN();
  SelectCellsArgs s = select_args(im, jm, km, i1, i2, j1, j2, k1, k2, d_a, a_is2d, d_b, b_is2d, b0, d_cells, cap, d_count);
  const DeviceInfo dev = use_device(-1);
  s.cells = d_cells;
  s.count = d_count;
  s.status = d_status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> g(g_cells_tables.mu);
  HIP_CHECK((hipError_t)launch_select_cells(s, cells_table(dev.ordinal, st), st));
  API_END();
}

int OHXSelectCells(int im, int jm, int km, int i1, int i2, int j1, int j2, int k1, int k2, const float* a, int a_is2d,
                   const float* b, int b_is2d, float b0, int64_t* cells, int64_t cap, int64_t* count) {
  API_BEGIN();
  SelectCellsArgs s = select_args(im, jm, km, i1, i2, j1, j2, k1, k2, a, a_is2d, b, b_is2d, b0, cells, cap, count);
  const int64_t nbox = s.wi * s.wj * s.wk;
  if (nbox == 0) {
    *count = 0;
    return 0;
  }
  const DeviceInfo dev = use_device(-1);
  hipStream_t st = lib_streams(dev.ordinal).exec;
  const int64_t plane = (int64_t)im * jm, off = plane * s.k0, slab = plane * s.wk;
  DevBuf<float> d_a, d_b;
  DevBuf<int64_t> d_cells, d_count;
  DevBuf<uint64_t> d_table;
  DevBuf<uint32_t> d_status;
  const int64_t keep = std::min(cap, nbox);
  d_cells.ensure((size_t)keep);
  d_count.ensure(1);
  d_table.ensure(kCellsMaxBlocks);
  d_status.ensure(1);
  // 3-D arrays: the box's levels only
  auto stage = [&](DevBuf<float>& d, const float* h, bool two_d) -> const float* {
    d.ensure((size_t)(two_d ? plane : slab));
    HIP_CHECK(hipMemcpyAsync(d.p, two_d ? h : h + off, (size_t)(two_d ? plane : slab) * sizeof(float),
                             hipMemcpyHostToDevice, st));
    return two_d ? d.p : slab_base(d.p, off);
  };
  if (s.a != nullptr) s.a = stage(d_a, a, s.a_is2d != 0);
  if (s.b != nullptr) s.b = stage(d_b, b, s.b_is2d != 0);
  s.cells = d_cells.p;
  s.count = d_count.p;
  s.status = d_status.p;
  HIP_CHECK(hipMemsetAsync(d_status.p, 0, sizeof(uint32_t), st));
  HIP_CHECK((hipError_t)launch_select_cells(s, d_table.p, st));
  int64_t found = 0;
  uint32_t status = 0;
  HIP_CHECK(hipMemcpyAsync(&found, d_count.p, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&status, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  const int64_t written = std::min(found, cap);
  if (written > 0) {
    HIP_CHECK(hipMemcpyAsync(cells, d_cells.p, (size_t)written * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }
  *count = found;
  if ((status & kCellsOverCap) != 0 || found > cap)
    throw OhxError("select_cells: " + std::to_string(found) + " cells are selected and cap is " + std::to_string(cap) +
                   ": the first " + std::to_string(cap) + " were written");
  API_END();
}

int OHXGatherCellsDevice(const float* const d_fields[], const int32_t is2d[], int nfield, int pl_feature, int im, int jm,
                         int km, const int64_t* d_cells, int64_t ncell, float* d_rows, uint32_t* d_status, void* stream) {
  API_BEGIN();
  const GatherCellsArgs g = gather_args(d_fields, is2d, nfield, pl_feature, im, jm, km, d_cells, ncell, d_rows);
  if (ncell == 0) return 0;
  (void)use_device(-1);
  HIP_CHECK((hipError_t)launch_gather_cells(g, d_cells, ncell, d_rows, d_status, static_cast<hipStream_t>(stream)));
  API_END();
}

int OHXGatherCells(const float* const fields[], const int32_t is2d[], int nfield, int pl_feature, int im, int jm, int km,
                   const int64_t* cells, int64_t ncell, float* rows) {
  API_BEGIN();
  GatherCellsArgs g = gather_args(fields, is2d, nfield, pl_feature, im, jm, km, cells, ncell, rows);
  if (ncell == 0) return 0;
  const DeviceInfo dev = use_device(-1);
  hipStream_t st = lib_streams(dev.ordinal).exec;
  // 3-D fields: only the levels the list's cells lie on cross PCIe
  int64_t lev0 = 0, lev1 = 0;
  const bool any = cells_level_range(cells, ncell, g.plane, g.ncells_total, &lev0, &lev1);
  const int64_t slab = any ? g.plane * (lev1 - lev0 + 1) : 0;
  const int64_t off3 = g.plane * lev0;
  std::vector<DevBuf<float>> d_field((size_t)nfield);
  DevBuf<int64_t> d_cells;
  DevBuf<float> d_rows;
  DevBuf<uint32_t> d_status;
  d_cells.ensure((size_t)ncell);
  d_rows.ensure((size_t)ncell * (size_t)nfield);
  d_status.ensure(1);
  for (int f = 0; f < nfield; ++f) {
    const int64_t n = !any ? 0 : (is2d[f] ? g.plane : slab);
    d_field[(size_t)f].ensure((size_t)n);
    if (n > 0)
      HIP_CHECK(hipMemcpyAsync(d_field[(size_t)f].p, is2d[f] ? fields[f] : fields[f] + off3, (size_t)n * sizeof(float),
                               hipMemcpyHostToDevice, st));
    g.field[f] = is2d[f] ? d_field[(size_t)f].p : slab_base(d_field[(size_t)f].p, off3);
  }
  HIP_CHECK(hipMemcpyAsync(d_cells.p, cells, (size_t)ncell * sizeof(int64_t), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemsetAsync(d_status.p, 0, sizeof(uint32_t), st));
  HIP_CHECK((hipError_t)launch_gather_cells(g, d_cells.p, ncell, d_rows.p, d_status.p, st));
  uint32_t status = 0;
  HIP_CHECK(hipMemcpyAsync(rows, d_rows.p, (size_t)ncell * (size_t)nfield * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&status, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  if ((status & kCellsOutOfRange) != 0) {
    int64_t at = 0;
    while (at < ncell && cells[at] >= 0 && cells[at] < g.ncells_total) ++at;
    throw OhxError("gather_cells: cell index out of range at position " + std::to_string(at) + " (" +
                   std::to_string(at < ncell ? cells[at] : 0) + ", the block has " + std::to_string(g.ncells_total) +
                   " cells): that row is NaN");
  }
  API_END();
}

int OHXScatterCellsDevice(const float* d_values, int64_t stride, int64_t col, const int64_t* d_cells, int64_t ncell,
                          float* d_out3d, int im, int jm, int km, uint32_t* d_status, void* stream) {
  API_BEGIN();
  scatter_check(d_values, stride, col, d_cells, ncell, d_out3d, im, jm, km);
  if (ncell == 0) return 0;
  const DeviceInfo dev = use_device(-1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> g(g_cells_tables.mu);
  HIP_CHECK((hipError_t)launch_scatter_cells(d_values, stride, col, d_cells, ncell, d_out3d, (int64_t)im * jm * km,
                                             d_status, cells_table(dev.ordinal, st), st));
  API_END();
}

int OHXScatterCells(const float* values, int64_t stride, int64_t col, const int64_t* cells, int64_t ncell, float* out3d,
                    int im, int jm, int km) {
  API_BEGIN();
  scatter_check(values, stride, col, cells, ncell, out3d, im, jm, km);
  if (ncell == 0) return 0;
  const DeviceInfo dev = use_device(-1);
  hipStream_t st = lib_streams(dev.ordinal).exec;
  const int64_t plane = (int64_t)im * jm, total = plane * km;
  // the column alone goes up, and of out3d only the levels the list's cells lie on go up and come back
  int64_t lev0 = 0, lev1 = 0;
  const bool any = cells_level_range(cells, ncell, plane, total, &lev0, &lev1);
  const int64_t off = plane * lev0, slab = any ? plane * (lev1 - lev0 + 1) : 0;
  std::vector<float> column((size_t)ncell);
  for (int64_t n = 0; n < ncell; ++n) column[(size_t)n] = values[n * stride + col];
  DevBuf<float> d_values, d_out;
  DevBuf<int64_t> d_cells;
  DevBuf<uint64_t> d_table;
  DevBuf<uint32_t> d_status;
  d_values.ensure((size_t)ncell);
  d_cells.ensure((size_t)ncell);
  d_out.ensure((size_t)slab);
  d_table.ensure(kCellsMaxBlocks);
  d_status.ensure(1);
  HIP_CHECK(hipMemcpyAsync(d_values.p, column.data(), (size_t)ncell * sizeof(float), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d_cells.p, cells, (size_t)ncell * sizeof(int64_t), hipMemcpyHostToDevice, st));
  if (any) HIP_CHECK(hipMemcpyAsync(d_out.p, out3d + off, (size_t)slab * sizeof(float), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemsetAsync(d_status.p, 0, sizeof(uint32_t), st));
  HIP_CHECK((hipError_t)launch_scatter_cells(d_values.p, 1, 0, d_cells.p, ncell, slab_base(d_out.p, off), total,
                                             d_status.p, d_table.p, st));
  uint32_t status = 0;
  if (any) HIP_CHECK(hipMemcpyAsync(out3d + off, d_out.p, (size_t)slab * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&status, d_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  if (status != 0) {
    int64_t top = INT64_MIN;
    for (int64_t n = 0; n < ncell; ++n) {
      const int64_t c = cells[n];
      if (c < 0 || c >= total)
        throw OhxError("scatter_cells: cell index out of range at position " + std::to_string(n) + " (" +
                       std::to_string(c) + ", the block has " + std::to_string(total) + " cells): skipped");
      if (c <= top)
        throw OhxError("scatter_cells: cells must be strictly ascending: position " + std::to_string(n) + " holds " +
                       std::to_string(c) + " after " + std::to_string(top) + ": skipped");
      top = c;
    }
    throw OhxError("scatter_cells: the kernel reported status " + std::to_string(status));
  }
  API_END();
}

// The host form's side of a tick (OHXBoosterRun1): its arrays cross PCIe in three lists on a copy stream, and
// run1_device says when - what the slab count needs first, what the feature engineering needs behind it, and the
// rest once the slab is known (of the sixteen fields only the walk reads, the slab's levels alone).
// Where the HOST spends a host-form tick (OHX_RUN1_TRACE=1 in the environment; measurement aid): microseconds since the
// call began at a few marks, printed for ticks 50 .. 52 of the process.
namespace {
struct TickTrace {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  std::vector<std::pair<const char*, double>> marks;
  void mark(const char* what) {
    marks.emplace_back(what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  void print(unsigned tick) const {
    std::string line = "[libohxgb] run1 tick " + std::to_string(tick) + " (host, us):";
    char buf[96];
    for (const auto& m : marks) {
      snprintf(buf, sizeof buf, " %s %.1f", m.first, m.second);
      line += buf;
    }
    fprintf(stderr, "%s\n", line.c_str());
  }
};
static thread_local TickTrace* g_tick_trace = nullptr;
#define TICK_MARK(what) do { if (g_tick_trace) g_tick_trace->mark(what); } while (0)

struct Run1Feed {
  virtual ~Run1Feed() = default;
  // each enqueues copies on the feed's own stream and returns an event recorded behind them
  virtual hipEvent_t slab_inputs() = 0;                              // PLE and TROPP of the model
  virtual hipEvent_t prep_inputs() = 0;                              // what the feature engineering reads
  virtual hipEvent_t walk_inputs(int k1, int k2) = 0;                // 1-based slab levels
  virtual hipEvent_t post_inputs() = 0;                              // what the tick's last kernel reads; asked for once the walk is enqueued
  // true when the slab count may read PLE and TROPP where the caller has them (registered arrays: *ple, *tropp = the
  // addresses the GPU reaches them at): it then waits for nothing, and their device copies - the tick's last kernel
  // reads them too - cross with prep_inputs(); slab_inputs() is not called
  virtual bool slab_in_place(const float** ple, const float** tropp) { (void)ple; (void)tropp; return false; }
  // true: a kernel that needs a list is launched when the HOST has seen the list's event, not enqueued behind a wait
  // on it (run1_device, below)
  virtual bool host_gated() const { return false; }
};
}  // namespace

// (both forms, before anything is staged or enqueued)
static void check_run1_shape(const OHXRun1Args& r) {
  if (r.im <= 0 || r.jm <= 0 || r.km <= 0) throw OhxError("OHXBoosterRun1: im, jm, km must be positive");
  if (r.km > kRun1MaxKm)
    throw OhxError("OHXBoosterRun1: km = " + std::to_string(r.km) + " levels; the limit is " + std::to_string(kRun1MaxKm));
}

static void run1_device(BoosterObj& b, const OHXRun1Args& r, hipStream_t stream, Run1Feed* feed = nullptr) {
  check_run1_shape(r);
  if (b.forest.num_feature != 27) throw OhxError("OHXBoosterRun1 needs the 27-feature OH booster");
  const void* need[] = {r.ple_mod, r.t_mod, r.q_mod, r.tropp_mod, r.ple_bst, r.zle_bst, r.tauclw, r.taucli,
                        r.gmito3, r.gmitto3, r.lat_deg, r.t_bst, r.no2, r.o3, r.ch4, r.co, r.isop, r.acet,
                        r.c2h6, r.c3h8, r.prpe, r.alk4, r.mp, r.h2o2, r.cloud, r.qv, r.albuv, r.ch2o, r.sza,
                        r.default_oh, r.oh};
  for (const void* p : need)
    if (p == nullptr) throw OhxError("OHXBoosterRun1: a required field pointer is NULL");
  for (int i = 0; i < 7; ++i)
    if (r.scacoef[i] == nullptr) throw OhxError("OHXBoosterRun1: a scattering-coefficient pointer is NULL");
  const size_t plane = (size_t)r.im * (size_t)r.jm, vol = plane * (size_t)r.km;
  for (int i = 0; i < 8; ++i) b.d_run1[i].ensure(i == 7 ? plane : vol);
  b.d_run1[8].ensure(vol);
  b.d_run1[9].ensure(vol);
  b.d_slab.ensure(2);
  // a DIAG buffer the caller gave IS the place the feature is built in; scratch otherwise
  auto or_scratch = [&](float* wanted, int slot) { return wanted ? wanted : b.d_run1[slot].p; };
  float* pl_bst = or_scratch(r.diag_pl_bst, 0);
  float *tauclwdn = or_scratch(r.diag_tauclwdn, 1), *tauclidn = or_scratch(r.diag_tauclidn, 2);
  float *taucliup = or_scratch(r.diag_taucliup, 3), *tauclwup = or_scratch(r.diag_tauclwup, 4);
  float *aodup = or_scratch(r.diag_aodup, 5), *aoddn = or_scratch(r.diag_aoddn, 6), *strato3 = or_scratch(r.diag_strato3, 7);
  float* oh_ml = or_scratch(r.oh_boost, 8);
  float* aod = or_scratch(r.diag_aod, 9);

  // ---- How a tick is laid out on the GPU (r5).  Two streams: the caller's, and a side stream of the booster's.
  //   side:   slab count (needs PLE and TROPP only) -> OH_ML := 0 -> [features of piece 1] -> after the walk of piece 0:
  //           post-processing of piece 0, [features of piece 2] -> ...
  //   main:   features of piece 0 -> (the host reads the slab count) -> walk of piece 0 -> walk of piece 1 -> ...
  // A PIECE is a range of j of the grid, all levels: the column sums need whole columns, the walk needs every feature
  // of the cells it walks, the mask and the unit conversion need the walk's OH_ML - and none of them needs another
  // column.  So of the streaming kernels (pointwise features, column sums, slab count, post-processing: 1.3 ms of a
  // C360 tick's 20.2 when they ran one after the other around the walk) only the first piece's features and the last
  // piece's post-processing are not hidden behind a walk, which leaves the CUs' spare registers and the whole of HBM's
  // bandwidth to them.  That was the plan; measured, pieces lose (below), so a tick is ONE piece unless ohx_run1_pieces > 1.
  if (!b.run1_fork) {
    HIP_CHECK(hipEventCreateWithFlags(&b.run1_fork, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&b.run1_slab, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&b.run1_join, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&b.run1_clear, hipEventDisableTiming));
  }
  b.h_slab.ensure(2);
  // The side stream.  Device form: the library's copy stream, idle there (the slab count runs beside the first
  // features: 0.19 ms of a C360 tick).  Host form: the copy stream carries the copies, and the side work goes to the
  // caller's stream in order - a third stream made a rank's tick slower alone (0.36-0.41 against 0.32 ms) and gave six
  // ranks on one GPU more queues than its scheduler maps at once (LibStreams; profiles/r05_sweeps.txt)
  hipStream_t side = (feed != nullptr || stream == b.s_copy) ? stream : b.s_copy;
  if (side != stream) {
    HIP_CHECK(hipEventRecord(b.run1_fork, stream));          // the side stream starts behind what the caller has enqueued
    HIP_CHECK(hipStreamWaitEvent(side, b.run1_fork, 0));
  }
  // host form: the slab count is the first thing of the tick.  Registered arrays: it reads PLE and TROPP over PCIe where
  // they are (0.34 MB of a rank's block; every edge once) and waits for no copy.  Else they cross first and it follows
  // them.  Either way its answer is back on the host while the features' inputs are still crossing, so the walk's own
  // inputs follow those over PCIe without a gap.
  SlabArgs sa;
  sa.im = r.im; sa.jm = r.jm; sa.km = r.km;
  sa.dynamic_k_range = r.dynamic_k_range; sa.tropp_min = r.tropp_min;
  sa.ple_mod = r.ple_mod; sa.tropp = r.tropp_mod; sa.result = b.d_slab.p;
  hipEvent_t prep_inputs = nullptr;
  const bool gated = feed != nullptr && feed->host_gated() && b.tune.run1_pieces <= 1;
  if (feed != nullptr) {
    if (!feed->slab_in_place(&sa.ple_mod, &sa.tropp)) {
      hipEvent_t ev = feed->slab_inputs();
      if (gated) HIP_CHECK(hipEventSynchronize(ev)); else HIP_CHECK(hipStreamWaitEvent(side, ev, 0));
    }
  }
  // (the result words are zero: set so when they were made, and again behind every read-back - a memset in front of the
  // count was a 12 us launch on the tick's critical path)
  // That trailing memset went to the side stream of ITS tick, and the device form returns with it still pending.  A tick
  // whose side stream is another one (device form, then host form; OHX_RUN1_STREAMS=1) must not count into words the old
  // memset has yet to clear - slab = 0, k1 = km + 1, nothing predicted, silently: it waits for run1_clear,
  // recorded behind that memset.
  if (!b.slab_zeroed) {
    HIP_CHECK(hipMemsetAsync(b.d_slab.p, 0, 2 * sizeof(int32_t), side));
    b.slab_zeroed = true;
  } else if (b.slab_zeroed_on != side) {
    HIP_CHECK(hipStreamWaitEvent(side, b.run1_clear, 0));
  }
  b.slab_zeroed_on = side;
  HIP_CHECK(launch_k_slab(sa, side));
  // ... and the next list is handed to the copy stream before this thread turns to anything else: the calls that
  // enqueue the rest of the slab count took it 50 us, during which the link stood idle (profiles/r05_sweeps.txt)
  if (feed != nullptr) prep_inputs = feed->prep_inputs();
  HIP_CHECK(hipMemcpyAsync(b.h_slab.p, b.d_slab.p, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, side));
  HIP_CHECK(hipEventRecord(b.run1_slab, side));
  HIP_CHECK(hipMemsetAsync(b.d_slab.p, 0, 2 * sizeof(int32_t), side));
  HIP_CHECK(hipEventRecord(b.run1_clear, side));
  HIP_CHECK(hipMemsetAsync(oh_ml, 0, vol * sizeof(float), side));            // self%OH_ML(:,:,:) = 0.0 (:1559)
  // A kernel that needs a list of the feed waits for it in one of two ways.  Enqueued behind a wait on the list's event
  // (hipStreamWaitEvent: a barrier packet on this queue that the command processor re-examines at its leisure - the
  // kernel behind it started 21-38 us after the copy had ended, profiles/r05_run1_timeline_block_48x24.txt), or GATED:
  // this thread waits for the event and launches then (a few us).  The feed says which.  Measured on a rank's tick: no
  // difference - the barriers' delay lies under the link's time (OHXBoosterRun1 below) - so nothing is gated by default.
  if (prep_inputs != nullptr && !gated) HIP_CHECK(hipStreamWaitEvent(stream, prep_inputs, 0));

  // pieces: ONE by default (ohx_run1_pieces 0 or 1).  n > 1 is an experiment knob: ranges of whole rows of bricks (four
  // j) walked one after the other, the pieces' extents independent of the slab count, which is not known yet.  Measured
  // (profiles/r05_sweeps.txt): more than one piece is slower - predict_fields_ring_kernel takes all of a CU's vector
  // registers (4 x 128 of 512 per SIMD), so a streaming kernel enqueued beside it waits for its end, and the pieces' own
  // launch tails cost 0.3 ms per C360 tick.
  const KernelKind kind = pick_kernel(b);
  int npieces = 1;
  if (kind == KernelKind::Ring && b.tune.run1_pieces > 1) npieces = std::max(1, std::min(b.tune.run1_pieces, r.jm / 8));
  std::vector<int> j_lo((size_t)npieces + 1, 0);
  for (int q = 1; q <= npieces; ++q) j_lo[(size_t)q] = q == npieces ? r.jm : (int)((int64_t)r.jm * q / npieces / 4 * 4);
  while (b.run1_prep.size() < (size_t)npieces) {
    hipEvent_t e1, e2;
    HIP_CHECK(hipEventCreateWithFlags(&e1, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&e2, hipEventDisableTiming));
    b.run1_prep.push_back(e1);
    b.run1_walk.push_back(e2);
  }

  PrepArgs pa;
  pa.im = r.im; pa.jm = r.jm; pa.km = r.km;
  pa.ple_bst = r.ple_bst; pa.zle_bst = r.zle_bst; pa.tauclw = r.tauclw; pa.taucli = r.taucli;
  for (int i = 0; i < 7; ++i) pa.sca[i] = r.scacoef[i];
  pa.gmito3 = r.gmito3; pa.gmitto3 = r.gmitto3;
  pa.pl_bst = pl_bst; pa.tauclwdn = tauclwdn; pa.tauclidn = tauclidn; pa.taucliup = taucliup; pa.tauclwup = tauclwup;
  pa.aodup = aodup; pa.aoddn = aoddn; pa.strato3 = strato3;
  auto prep_piece = [&](int q, hipStream_t s) {
    PrepArgs p = pa;
    p.beside_a_walk = q >= 2 ? 1 : 0;        // pieces 0 and 1 are prepared before the first walk starts
    if (npieces > 1) {
      p.col0 = (uint64_t)j_lo[(size_t)q] * (uint64_t)r.im;
      p.ncols = (uint64_t)(j_lo[(size_t)q + 1] - j_lo[(size_t)q]) * (uint64_t)r.im;
    }
    HIP_CHECK(launch_feature_prep(p, aod, s));
  };
  PostArgs po;
  po.im = r.im; po.jm = r.jm; po.km = r.km;
  po.avogad = r.avogad; po.runiv = r.runiv; po.epsilon = r.epsilon;
  po.ple_mod = r.ple_mod; po.t_mod = r.t_mod; po.q_mod = r.q_mod; po.tropp = r.tropp_mod;
  po.default_oh = r.default_oh; po.oh_ml = oh_ml; po.oh = r.oh; po.ndwet = r.ndwet;
  auto post_piece = [&](int q, hipStream_t s) {
    PostArgs p = po;
    if (npieces > 1) {
      p.col0 = (uint64_t)j_lo[(size_t)q] * (uint64_t)r.im;
      p.ncols = (uint64_t)(j_lo[(size_t)q + 1] - j_lo[(size_t)q]) * (uint64_t)r.im;
    }
    HIP_CHECK(launch_post_process(p, s));
  };

  if (!gated) prep_piece(0, stream);
  if (npieces > 1) {
    if (prep_inputs != nullptr && side != stream) HIP_CHECK(hipStreamWaitEvent(side, prep_inputs, 0));      // later pieces' features run here
    prep_piece(1, side);
    HIP_CHECK(hipEventRecord(b.run1_prep[1], side));
  }
  // the one wait in the middle of a tick: the slab count sizes the walk's launches (and the reference asserts on it,
  // :287-288); it was enqueued before everything else of this tick and the features are being computed meanwhile
  TICK_MARK("features-enqueued");
  HIP_CHECK(hipEventSynchronize(b.run1_slab));
  TICK_MARK("slab-known");
  const int32_t slab[2] = {b.h_slab.p[0], b.h_slab.p[1]};
  if (!r.dynamic_k_range && slab[1] != 0) {
    (void)hipStreamSynchronize(side);
    (void)hipStreamSynchronize(stream);
    throw OhxError("OH Prediction: Minimum tropopause pressure is not low enough!");
  }
  const int k1 = r.km - slab[0] + 1, k2 = r.km;   // 1-based (:300-301)
  if (r.k1) *r.k1 = k1;
  if (r.k2) *r.k2 = k2;
  hipEvent_t post_inputs = nullptr, walk_inputs = nullptr;
  if (feed != nullptr) walk_inputs = feed->walk_inputs(k1, k2);
  TICK_MARK("walk-inputs-enqueued");
  if (gated) {
    // (the walk's list is on its way before this thread waits for the features': the link is not idle meanwhile)
    HIP_CHECK(hipEventSynchronize(prep_inputs));
    prep_piece(0, stream);
    TICK_MARK("features-launched");
  } else if (walk_inputs != nullptr) {
    HIP_CHECK(hipStreamWaitEvent(stream, walk_inputs, 0));
  }

  const float* fields[27] = {r.lat_deg, pl_bst, r.t_bst, r.no2, r.o3, r.ch4, r.co, r.isop, r.acet, r.c2h6, r.c3h8,
                             r.prpe, r.alk4, r.mp, r.h2o2, tauclwdn, tauclidn, taucliup, tauclwup, r.cloud, r.qv,
                             strato3, r.albuv, aodup, aoddn, r.ch2o, r.sza};      // order of :313-339
  static const int32_t is2d[27] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1};
  if (kind == KernelKind::Wide) ensure_wide(b);
  // OH_ML := 0 (side stream) lies before the first store of a walk
  if (side != stream) {
    HIP_CHECK(hipEventRecord(b.run1_join, side));
    HIP_CHECK(hipStreamWaitEvent(stream, b.run1_join, 0));
  }
  for (int q = 0; q < npieces; ++q) {
    const int jq = j_lo[(size_t)q + 1] - j_lo[(size_t)q];
    const uint64_t first = (uint64_t)j_lo[(size_t)q] * (uint64_t)r.im;        // the piece's first column
    if (q >= 1) HIP_CHECK(hipStreamWaitEvent(stream, b.run1_prep[(size_t)q], 0));      // its features are there
    if (k2 >= k1 && jq > 0) {
      FieldsArgs fa{};
      fa.is2d_mask = 0;
      for (int f = 0; f < 27; ++f) {
        fa.field[f] = fields[f] + first;
        if (is2d[f]) fa.is2d_mask |= (1u << f);
      }
      fa.pl_feature = 1;
      fa.nfield = 27;
      fa.im = r.im; fa.jm = jq; fa.km = r.km;
      fa.level_stride = npieces > 1 ? plane : 0;
      fa.k1 = k1 - 1; fa.k2 = k2 - 1;
      fa.missing = r.missing;
      tree_range(b, 0, &fa.tree_begin, &fa.tree_end);
      fa.apply_pow10 = 1;
      fa.scale = r.ohscale;
      fa.out = oh_ml + first;
      fa.flags = b.d_flags.p;
      const uint64_t slab_rows = (uint64_t)r.im * (uint64_t)jq * (uint64_t)(k2 - k1 + 1);
      // (not walk_with_buffers: the gated wait for the walk's inputs sits between the list's set-up and the launch, and only
      // the last piece's count is looked at)
      LaunchTuning tune = b.tune;
      leaf_room(b, slab_rows, fa.tree_end - fa.tree_begin, tune, r.im, jq, 0);
      const bool deferring = defer_prepare(b, slab_rows, tune, stream);
      if (gated && q == 0) {
        HIP_CHECK(hipEventSynchronize(walk_inputs));
        TICK_MARK("walk-inputs-there");
      }
      HIP_CHECK(launch_predict_fields(kind, device_forest(b), fa, b.dev.num_cus, stream, tune));
      if (deferring && q + 1 == npieces) defer_look(b, slab_rows, stream);
    }
    TICK_MARK("walk-enqueued");
    if (feed != nullptr && post_inputs == nullptr) post_inputs = feed->post_inputs();      // behind the (first) walk's launch
    if (npieces == 1) {
      if (post_inputs != nullptr) HIP_CHECK(hipStreamWaitEvent(stream, post_inputs, 0));
      post_piece(0, stream);
      break;
    }
    // the piece is walked: its mask and unit conversion, then the features of the piece after next, beside the next walk
    HIP_CHECK(hipEventRecord(b.run1_walk[(size_t)q], stream));
    HIP_CHECK(hipStreamWaitEvent(side, b.run1_walk[(size_t)q], 0));
    if (post_inputs != nullptr) HIP_CHECK(hipStreamWaitEvent(side, post_inputs, 0));
    post_piece(q, side);
    if (q + 2 < npieces) {
      prep_piece(q + 2, side);
      HIP_CHECK(hipEventRecord(b.run1_prep[(size_t)q + 2], side));
    }
  }
  if (npieces > 1 && side != stream) {       // the caller's stream ends behind everything the side stream did
    HIP_CHECK(hipEventRecord(b.run1_join, side));
    HIP_CHECK(hipStreamWaitEvent(stream, b.run1_join, 0));
  }
}

int OHXBoosterRun1Device(BoosterHandle handle, const OHXRun1Args* args, void* stream) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  refuse_groups(*b, "OHXBoosterRun1Device");
  refuse_categorical(*b, "OHXBoosterRun1Device");
  if (args == nullptr) throw OhxError("OHXBoosterRun1Device: args is NULL");
  if (!objective_is_identity(b->forest.objective))
    throw OhxError("objective '" + b->forest.objective + "' is not supported by OHXBoosterRun1");
  ensure_uploaded(*b);
  run1_device(*b, *args, static_cast<hipStream_t>(stream));
  API_END();
}

static PostArgs post_args(int im, int jm, int km, float avogad, float runiv, float epsilon, const float* ple_mod,
                          const float* t_mod, const float* q_mod, const float* tropp_mod, const float* default_oh,
                          const float* oh_ml, float* oh, float* ndwet) {
  if (im <= 0 || jm <= 0 || km <= 0) throw OhxError("OHXOHPostProcess: im, jm, km must be positive");
  if (!ple_mod || !t_mod || !q_mod || !tropp_mod || !default_oh || !oh_ml || !oh)
    throw OhxError("OHXOHPostProcess: a required field pointer is NULL");
  PostArgs po;
  po.im = im; po.jm = jm; po.km = km;
  po.avogad = avogad; po.runiv = runiv; po.epsilon = epsilon;
  po.ple_mod = ple_mod; po.t_mod = t_mod; po.q_mod = q_mod; po.tropp = tropp_mod;
  po.default_oh = default_oh; po.oh_ml = oh_ml; po.oh = oh; po.ndwet = ndwet;
  return po;
}

int OHXOHPostProcessDevice(int im, int jm, int km, float avogad, float runiv, float epsilon, const float* d_ple_mod,
                           const float* d_t_mod, const float* d_q_mod, const float* d_tropp_mod,
                           const float* d_default_oh, const float* d_oh_ml, float* d_oh, float* d_ndwet, void* stream) {
  API_BEGIN();
  (void)use_device(-1);
  HIP_CHECK(launch_post_process(post_args(im, jm, km, avogad, runiv, epsilon, d_ple_mod, d_t_mod, d_q_mod, d_tropp_mod,
                                          d_default_oh, d_oh_ml, d_oh, d_ndwet), static_cast<hipStream_t>(stream)));
  API_END();
}

namespace {
// staging of the host form: one set of device buffers per process, reused from tick to tick
struct PostScratch {
  std::mutex mu;
  int device = -1;
  DevBuf<float> buf[8];
};
static PostScratch g_post;   // static: inside extern "C" an unnamed namespace alone does not keep the name out of the dynamic table
}  // namespace

int OHXOHPostProcess(int im, int jm, int km, float avogad, float runiv, float epsilon, const float* ple_mod,
                     const float* t_mod, const float* q_mod, const float* tropp_mod, const float* default_oh,
                     const float* oh_ml, float* oh, float* ndwet) {
  API_BEGIN();
  (void)post_args(im, jm, km, avogad, runiv, epsilon, ple_mod, t_mod, q_mod, tropp_mod, default_oh, oh_ml, oh, ndwet);
  const DeviceInfo dev = use_device(-1);
  const size_t plane = (size_t)im * (size_t)jm, vol = plane * (size_t)km, edge = plane * (size_t)(km + 1);
  std::lock_guard<std::mutex> g(g_post.mu);
  if (g_post.device != dev.ordinal) {
    for (auto& bf : g_post.buf) bf.release();
    g_post.device = dev.ordinal;
  }
  const float* src[6] = {ple_mod, t_mod, q_mod, tropp_mod, default_oh, oh_ml};
  const size_t n[6] = {edge, vol, vol, plane, vol, vol};
  hipStream_t st = lib_streams(dev.ordinal).exec;
  HostMover in(st, true);
  for (int i = 0; i < 6; ++i) {
    g_post.buf[i].ensure(n[i]);
    in.add(g_post.buf[i].p, src[i], n[i]);
  }
  in.go();
  g_post.buf[6].ensure(vol);
  if (ndwet) g_post.buf[7].ensure(vol);
  HIP_CHECK(launch_post_process(post_args(im, jm, km, avogad, runiv, epsilon, g_post.buf[0].p, g_post.buf[1].p,
                                          g_post.buf[2].p, g_post.buf[3].p, g_post.buf[4].p, g_post.buf[5].p,
                                          g_post.buf[6].p, ndwet ? g_post.buf[7].p : nullptr), st));
  HostMover back(st, false);
  back.add(oh, g_post.buf[6].p, vol);
  if (ndwet) back.add(ndwet, g_post.buf[7].p, vol);
  back.go();
  HIP_CHECK(hipStreamSynchronize(st));
  API_END();
}

int OHXJulianDay(int nymd, int* jday) {
  API_BEGIN();
  if (jday == nullptr) throw OhxError("OHXJulianDay: jday is NULL");
  static const int days[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  const int ny = nymd / 10000, mm = (nymd % 10000) / 100, dd = nymd % 100;
  // leap_year (:1940-1970): no leap years before year 0
  const bool leap = ny >= 0 && ((ny % 100 == 0 && ny % 400 == 0) || (ny % 4 == 0 && ny % 100 != 0));
  int ds = dd;
  for (int m = 1; m < mm && m <= 12; ++m) ds += (m == 2 && leap) ? 29 : days[m - 1];
  *jday = ds;
  API_END();
}

int OHXSolarGeometryDevice(int jday, const float* d_lats, const float* d_lons, int im, int jm, float deg2rad,
                           float rad2deg, float* d_lat_deg, float* d_sza_noon, void* stream) {
  API_BEGIN();
  if (im < 0 || jm < 0) throw OhxError("OHXSolarGeometry: im and jm must not be negative");
  if ((size_t)im * (size_t)jm != 0 && (d_lats == nullptr || (d_sza_noon != nullptr && d_lons == nullptr)))
    throw OhxError("OHXSolarGeometry: LATS (and LONS, for the zenith angle) must not be NULL");
  use_device(-1);
  SolarArgs a;
  a.im = im; a.jm = jm; a.jday = jday;
  a.deg2rad = deg2rad; a.rad2deg = rad2deg;
  a.lats = d_lats; a.lons = d_lons;
  a.lat_deg = d_lat_deg; a.sza_noon = d_sza_noon;
  HIP_CHECK(launch_solar_geometry(a, static_cast<hipStream_t>(stream)));
  API_END();
}

int OHXSolarGeometry(int jday, const float* lats, const float* lons, int im, int jm, float deg2rad, float rad2deg,
                     float* lat_deg, float* sza_noon) {
  API_BEGIN();
  if (im < 0 || jm < 0) throw OhxError("OHXSolarGeometry: im and jm must not be negative");
  const size_t plane = (size_t)im * (size_t)jm;
  if (plane == 0) return 0;
  if (lats == nullptr || (sza_noon != nullptr && lons == nullptr))
    throw OhxError("OHXSolarGeometry: LATS (and LONS, for the zenith angle) must not be NULL");
  const DeviceInfo dev = use_device(-1);
  hipStream_t st = lib_streams(dev.ordinal).exec;
  DevBuf<float> d_lats, d_lons, d_lat, d_sza;
  d_lats.ensure(plane);
  HIP_CHECK(hipMemcpyAsync(d_lats.p, lats, plane * sizeof(float), hipMemcpyHostToDevice, st));
  if (sza_noon) {
    d_lons.ensure(plane);
    HIP_CHECK(hipMemcpyAsync(d_lons.p, lons, plane * sizeof(float), hipMemcpyHostToDevice, st));
    d_sza.ensure(plane);
  }
  if (lat_deg) d_lat.ensure(plane);
  SolarArgs a;
  a.im = im; a.jm = jm; a.jday = jday;
  a.deg2rad = deg2rad; a.rad2deg = rad2deg;
  a.lats = d_lats.p; a.lons = d_lons.p;
  a.lat_deg = lat_deg ? d_lat.p : nullptr;
  a.sza_noon = sza_noon ? d_sza.p : nullptr;
  HIP_CHECK(launch_solar_geometry(a, st));
  if (lat_deg) HIP_CHECK(hipMemcpyAsync(lat_deg, d_lat.p, plane * sizeof(float), hipMemcpyDeviceToHost, st));
  if (sza_noon) HIP_CHECK(hipMemcpyAsync(sza_noon, d_sza.p, plane * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));        // before the device buffers go
  API_END();
}

int OHXBoosterRun1(BoosterHandle handle, const OHXRun1Args* args) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  refuse_groups(*b, "OHXBoosterRun1");
  refuse_categorical(*b, "OHXBoosterRun1");
  if (args == nullptr) throw OhxError("OHXBoosterRun1: args is NULL");
  if (!objective_is_identity(b->forest.objective))
    throw OhxError("objective '" + b->forest.objective + "' is not supported by OHXBoosterRun1");
  ensure_uploaded(*b);
  const OHXRun1Args& h = *args;
  check_run1_shape(h);
  const size_t plane = (size_t)h.im * (size_t)h.jm, vol = plane * (size_t)h.km, edge = plane * (size_t)(h.km + 1);
  OHXRun1Args d = h;
  // Every input goes to HBM once, in the order the tick needs it (Run1Feed): stage 0 = what the slab count reads,
  // 1 = what the feature engineering reads, 3 = what only the walk reads - sixteen 3-D fields, of which the slab's
  // levels cross, once the slab is known, and three 2-D ones - 2 = what the last kernel of the tick reads (the model's
  // own T, Q and the default OH, on every level), which crosses last, under the walk (a 48 x 24 x 72 block: 51 of 72 levels, 1.5 of 10.3 MB less over PCIe).  An array that
  // is passed twice (ONLINE_INST: T is both the model's and Boost's, OH_GridCompMod.F90:1326-1349) crosses once.
  struct In { const float* host; const float** dev; size_t n; int stage; };
  In ins[] = {
      {h.ple_mod, &d.ple_mod, edge, 0}, {h.tropp_mod, &d.tropp_mod, plane, 0},
      {h.ple_bst, &d.ple_bst, edge, 1}, {h.zle_bst, &d.zle_bst, edge, 1}, {h.tauclw, &d.tauclw, vol, 1}, {h.taucli, &d.taucli, vol, 1},
      {h.scacoef[0], &d.scacoef[0], vol, 1}, {h.scacoef[1], &d.scacoef[1], vol, 1}, {h.scacoef[2], &d.scacoef[2], vol, 1},
      {h.scacoef[3], &d.scacoef[3], vol, 1}, {h.scacoef[4], &d.scacoef[4], vol, 1}, {h.scacoef[5], &d.scacoef[5], vol, 1},
      {h.scacoef[6], &d.scacoef[6], vol, 1}, {h.gmito3, &d.gmito3, plane, 1}, {h.gmitto3, &d.gmitto3, plane, 1},
      {h.t_mod, &d.t_mod, vol, 2}, {h.q_mod, &d.q_mod, vol, 2}, {h.default_oh, &d.default_oh, vol, 2},
      {h.lat_deg, &d.lat_deg, plane, 3}, {h.albuv, &d.albuv, plane, 3}, {h.sza, &d.sza, plane, 3},
      {h.t_bst, &d.t_bst, vol, 3}, {h.no2, &d.no2, vol, 3}, {h.o3, &d.o3, vol, 3}, {h.ch4, &d.ch4, vol, 3}, {h.co, &d.co, vol, 3},
      {h.isop, &d.isop, vol, 3}, {h.acet, &d.acet, vol, 3}, {h.c2h6, &d.c2h6, vol, 3}, {h.c3h8, &d.c3h8, vol, 3},
      {h.prpe, &d.prpe, vol, 3}, {h.alk4, &d.alk4, vol, 3}, {h.mp, &d.mp, vol, 3}, {h.h2o2, &d.h2o2, vol, 3},
      {h.cloud, &d.cloud, vol, 3}, {h.qv, &d.qv, vol, 3}, {h.ch2o, &d.ch2o, vol, 3}};
  constexpr size_t nin = sizeof(ins) / sizeof(ins[0]);
  if (b->d_run1_stage.size() < nin + 3 + 9) b->d_run1_stage.resize(nin + 3 + 9);
  // an array handed over twice is staged once: the later entry takes the earlier one's device copy - and its stage,
  // if that one crosses in full (a stage-3 entry shares only with a full copy, never the other way round)
  int same_as[nin];
  bool whole[nin];                       // crosses in full even at stage 3
  for (size_t i = 0; i < nin; ++i) whole[i] = ins[i].stage != 3 || ins[i].n == plane;
  for (size_t i = 0; i < nin; ++i) {
    if (ins[i].host == nullptr) throw OhxError("OHXBoosterRun1: a required field pointer is NULL");
    same_as[i] = -1;
    for (size_t q = 0; q < i && same_as[i] < 0; ++q)
      if (ins[q].host == ins[i].host && ins[q].n == ins[i].n && same_as[q] < 0 && ins[q].stage != 3) same_as[i] = (int)q;
    if (same_as[i] >= 0) {
      *ins[i].dev = b->d_run1_stage[(size_t)same_as[i]].p;
      // the walk reads it too: it crosses with the walk's inputs, in full (ins[q].n == vol keeps it whole below)
      if (ins[i].stage == 3 && ins[(size_t)same_as[i]].stage == 2) {
        ins[(size_t)same_as[i]].stage = 3;
        whole[(size_t)same_as[i]] = true;
      }
      continue;
    }
    b->d_run1_stage[i].ensure(ins[i].n);
    *ins[i].dev = b->d_run1_stage[i].p;
  }
  struct Feed : Run1Feed {
    BoosterObj* b;
    In* ins;
    const int* same_as;
    const bool* whole;
    size_t plane, km;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t post_blocks = 0;
    bool post_by_dma = false, all_by_dma = false;
    void stage(int which, int k1, int k2) {
      HostMover in(b->s_copy, true);
      in.by_dma = all_by_dma;
      if (which == 2) {
        in.blocks_override = post_blocks;
        in.by_dma = post_by_dma || all_by_dma;
      }
      for (size_t i = 0; i < nin; ++i) {
        if (ins[i].stage != which || same_as[i] >= 0) continue;
        float* dev = b->d_run1_stage[i].p;
        if (!whole[i]) {
          if (k2 >= k1) in.add_slice(dev + plane * (size_t)(k1 - 1), ins[i].host, plane * km, plane * (size_t)(k1 - 1), plane * (size_t)(k2 - k1 + 1));
        } else {
          in.add(dev, ins[i].host, ins[i].n);
        }
      }
      in.go();
    }
    hipEvent_t slab_inputs() override {
      stage(0, 0, 0);
      HIP_CHECK(hipEventRecord(ev[0], b->s_copy));
      return ev[0];
    }
    hipEvent_t prep_inputs() override {
      stage(1, 0, 0);
      HIP_CHECK(hipEventRecord(ev[1], b->s_copy));
      return ev[1];
    }
    hipEvent_t walk_inputs(int k1, int k2) override {
      stage(3, k1, k2);
      HIP_CHECK(hipEventRecord(ev[2], b->s_copy));
      return ev[2];
    }
    hipEvent_t post_inputs() override {          // the model's T, Q and the default OH cross under the walk
      stage(2, 0, 0);
      HIP_CHECK(hipEventRecord(ev[3], b->s_copy));
      return ev[3];
    }
    bool in_place = true, gate = false;
    bool slab_in_place(const float** ple, const float** tropp) override {
      if (!in_place) return false;
      void *mp = nullptr, *mt = nullptr;           // ins[0], ins[1]: the model's PLE and TROPP
      if (!g_host_registry.want(ins[0].host, ins[0].n * sizeof(float), &mp) || mp == nullptr) return false;
      if (!g_host_registry.want(ins[1].host, ins[1].n * sizeof(float), &mt) || mt == nullptr) return false;
      *ple = static_cast<const float*>(mp);
      *tropp = static_cast<const float*>(mt);
      ins[0].stage = ins[1].stage = 1;             // their device copies (the last kernel's) cross with the next list
      return true;
    }
    bool host_gated() const override { return gate; }
  } feed;
  feed.b = b;
  feed.ins = ins;
  feed.same_as = same_as;
  feed.whole = whole;
  feed.plane = plane;
  feed.km = (size_t)h.km;
  while (b->run1_feed_events.size() < 4) {
    hipEvent_t e;
    // with timing: such a record is a packet with a completion signal of its own.  Recorded without, the waits on these
    // events were released by the NEXT copy's end (the feature kernels started when list B had landed, 80 us late:
    // profiles/r05_sweeps.txt)
    HIP_CHECK(hipEventCreate(&e));
    b->run1_feed_events.push_back(e);
  }
  for (int i = 0; i < 4; ++i) feed.ev[i] = b->run1_feed_events[(size_t)i];
  if (h.oh == nullptr) throw OhxError("OHXBoosterRun1: oh is NULL");
  b->d_run1_stage[nin].ensure(vol);
  d.oh = b->d_run1_stage[nin].p;
  d.ndwet = nullptr;
  if (h.ndwet) {
    b->d_run1_stage[nin + 1].ensure(vol);
    d.ndwet = b->d_run1_stage[nin + 1].p;
  }
  d.oh_boost = nullptr;
  if (h.oh_boost) {
    b->d_run1_stage[nin + 2].ensure(vol);
    d.oh_boost = b->d_run1_stage[nin + 2].p;
  }
  // DIAG dumps: device copies only for the ones asked for
  struct Out { float* host; float** dev; size_t n; };
  Out outs[] = {{h.diag_pl_bst, &d.diag_pl_bst, vol}, {h.diag_tauclwdn, &d.diag_tauclwdn, vol},
                {h.diag_tauclidn, &d.diag_tauclidn, vol}, {h.diag_taucliup, &d.diag_taucliup, vol},
                {h.diag_tauclwup, &d.diag_tauclwup, vol}, {h.diag_aodup, &d.diag_aodup, vol},
                {h.diag_aoddn, &d.diag_aoddn, vol}, {h.diag_aod, &d.diag_aod, vol}, {h.diag_strato3, &d.diag_strato3, plane}};
  const size_t nout = sizeof(outs) / sizeof(outs[0]);
  if (b->d_run1_stage.size() < nin + 3 + nout) b->d_run1_stage.resize(nin + 3 + nout);
  for (size_t i = 0; i < nout; ++i) {
    *outs[i].dev = nullptr;
    if (outs[i].host == nullptr) continue;
    b->d_run1_stage[nin + 3 + i].ensure(outs[i].n);
    *outs[i].dev = b->d_run1_stage[nin + 3 + i].p;
  }
  // experiment knobs, read once (profiles/r05_sweeps.txt has what each is worth): OHX_RUN1_STREAMS=1 puts the copies on
  // the kernels' stream; OHX_RUN1_GATE=1 launches every kernel when this thread has seen its list's event instead of
  // enqueueing it behind a wait on the event; OHX_RUN1_SLAB_IN_PLACE=1 lets the slab count read PLE and TROPP over PCIe
  static const int nstreams = [] { const char* e = getenv("OHX_RUN1_STREAMS"); return e ? atoi(e) : 2; }();
  // (both measured worth nothing on a rank's block - 0.312 ms off / off, 0.314 in place, 0.319 gated and in place: the front
  // of a tick is bound by the link, 9.4 MB in 178 us, whatever the kernels wait for - and so both are off)
  static const bool knob_gate = [] { const char* e = getenv("OHX_RUN1_GATE"); return e && e[0] == '1'; }();
  static const bool knob_in_place = [] { const char* e = getenv("OHX_RUN1_SLAB_IN_PLACE"); return e && e[0] == '1'; }();
  feed.gate = knob_gate && nstreams != 1 && g_host_registry.on.load(std::memory_order_relaxed);
  feed.in_place = knob_in_place;
  // The last list of a tick (what only the mask and the conversion read) crosses UNDER the walk, and a copy kernel is bad
  // company for a walk: with the usual 64 blocks the walk "started" when the 20 us copy ended (its packet and arguments are
  // fetched over the link, behind the copy's queued reads), with 8 blocks it started at once and took 116 us instead of 66
  // (waves that share a CU with copy waves waiting on PCIe wait with them: a CU's vector memory path returns in order)
  // (profiles/r05_run1_timeline_block_48x24.txt, r05_sweeps.txt: "copy kernels on CUs of their own" tells the two apart).  So
  // this one list goes through the DMA engines (three hipMemcpyAsync of registered arrays, 11 us each, no wave on any
  // CU): a rank's tick 0.301 -> 0.293-0.297 ms.  OHX_COPY_POST_BLOCKS (read once): -1 = DMA (default), 0 = a copy kernel
  // like the other lists, n = one of n blocks.
  static const int knob_post_blocks = [] { const char* e = getenv("OHX_COPY_POST_BLOCKS"); return e ? atoi(e) : -1; }();
  feed.post_blocks = knob_post_blocks > 0 ? (uint32_t)knob_post_blocks : 0u;
  feed.post_by_dma = knob_post_blocks < 0;
  // ohx_copy_engine: dma, or auto's verdict (or its trial's turn) for a tick on registered arrays
  const int engine = g_copy_engine.load(std::memory_order_relaxed);
  const bool trying = engine == kCopyAuto && g_host_registry.on.load(std::memory_order_relaxed);
  feed.all_by_dma = engine == kCopyDma || (trying && b->copy_trial.dma_now(vol));
  const auto tick_began = std::chrono::steady_clock::now();
  hipStream_t main = nstreams == 1 ? b->s_copy : b->s_exec;
  // OHX_RUN1_TRACE=<n> (1 = 50): the host's time marks of ticks n .. n + 2 of this process on stderr
  static const int trace_from = [] { const char* e = getenv("OHX_RUN1_TRACE"); const int n = e ? atoi(e) : -1; return n == 1 ? 50 : n; }();
  const bool tracing = trace_from >= 0;
  static std::atomic<unsigned> tick_no{0};
  TickTrace trace;
  // however this call ends - judge_flags / raise_flag_errors throw after the read-back too - the thread's pointer to
  // `trace` does not outlive it
  struct TraceReset { ~TraceReset() { g_tick_trace = nullptr; } } trace_reset;
  const unsigned tick = tick_no.fetch_add(1);
  g_tick_trace = (tracing && tick >= (unsigned)trace_from && tick <= (unsigned)trace_from + 2u) ? &trace : nullptr;
  TICK_MARK("set-up");
  try {
    run1_device(*b, d, main, &feed);
  } catch (...) {
    // nothing of this call may still be reading the caller's arrays when it returns, error or not
    (void)hipStreamSynchronize(b->s_copy);
    (void)hipStreamSynchronize(main);
    g_tick_trace = nullptr;
    throw;
  }
  HostMover back(main, false);
  back.by_dma = feed.all_by_dma;
  back.add(h.oh, d.oh, vol);
  if (h.ndwet) back.add(h.ndwet, d.ndwet, vol);
  if (h.oh_boost) back.add(h.oh_boost, d.oh_boost, vol);
  for (size_t i = 0; i < nout; ++i)
    if (outs[i].host) back.add(outs[i].host, *outs[i].dev, outs[i].n);
  // the kernels' flag words come back on the same launch (a read-back of their own was one more launch at a tick's end)
  b->h_flags.ensure(2);
  void* flags_there = nullptr;          // where the GPU reaches the pinned words
  if (hipHostGetDevicePointer(&flags_there, b->h_flags.p, 0) != hipSuccess) {
    (void)hipGetLastError();
    flags_there = nullptr;
  }
  const bool flags_ride = flags_there != nullptr && back.ride(flags_there, b->d_flags.p, 2);
  back.go();
  TICK_MARK("all-enqueued");
  if (flags_ride) {
    HIP_CHECK(hipStreamSynchronize(main));          // the outputs are in the caller's arrays
    const uint32_t flags[2] = {b->h_flags.p[0], b->h_flags.p[1]};
    judge_flags(*b, flags, main);
  } else {
    raise_flag_errors(*b, main);        // waits for the stream
  }
  TICK_MARK("done");
  if (trying) b->copy_trial.report(feed.all_by_dma, std::chrono::duration<double>(std::chrono::steady_clock::now() - tick_began).count());
  if (g_tick_trace) g_tick_trace->print(tick);
  g_tick_trace = nullptr;
  API_END();
}

int OHXBoosterGetInfo(BoosterHandle handle, bst_ulong info[8]) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  if (info == nullptr) throw OhxError("OHXBoosterGetInfo: info is NULL");
  if (!b->loaded) throw OhxError("the booster holds no model");
  if (b->num_cat != 0) {
    // categorical splits: node format 3 (flatten.hpp CatNode); host-only like the rest
    Placement lp = b->uploaded ? Placement() : place_forest(b->forest, b->layout);
    const Placement& pl = b->uploaded ? b->placement : lp;
    uint64_t words = b->cat_word_count;
    if (!b->uploaded) words = emit_cat(b->forest, pl).words.size();
    info[0] = b->forest.trees.size();
    info[1] = pl.real_nodes;
    info[2] = pl.num_slots;
    info[3] = pl.num_slots * sizeof(CatNode) + words * sizeof(uint32_t);
    info[4] = (bst_ulong)pl.max_depth;
    info[5] = b->forest.num_feature;
    info[6] = 3;
    info[7] = 0;
    return 0;
  }
  // host-only: placement can be computed without a device
  Placement local;
  const Placement* p = &b->placement;
  bool packed_ok = b->packed_ok;
  if (!b->uploaded) {
    local = place_forest(b->forest, b->layout);
    p = &local;
    packed_ok = packed_format_fits(b->forest, local);
  }
  const bool packed_used = packed_ok && b->kernel_name != "wide";
  bool super_used = false;
  uint64_t super_slots = b->super_slots;
  // (the ring kernels where the booster's big batches go through them: pick_kernel)
  auto walk_mode = [&](double mean_steps) {
    const bool ring = b->kernel_name == "ring" ||
                      (b->kernel_name == "auto" && b->forest.num_feature == 27 && mean_steps >= kRingMinMeanSteps);
    return ring ? 2 : (use_tree_tops(b->tune, mean_steps) ? 1 : 0);
  };
  uint64_t super_gathers = b->super_gathers[walk_mode(b->super_mean_steps)];
  if (wants_super(b->kernel_name)) {
    if (b->uploaded) {
      super_used = b->super_ok;
    } else {
      SuperForest sf;
      super_used = emit_super(b->forest, &sf, b->layout.super_pack);
      super_slots = sf.nodes.size();
      super_gathers = count_super_gathers(sf, walk_mode(mean_super_steps(sf)));
    }
  }
  info[0] = b->forest.trees.size();
  info[1] = p->real_nodes;
  info[2] = super_used ? super_slots : p->num_slots;
  info[3] = super_used ? super_slots * sizeof(SuperNode)
                       : p->num_slots * (packed_used ? sizeof(PackedNode) : sizeof(WideNode));
  info[4] = (bst_ulong)p->max_depth;
  info[5] = b->forest.num_feature;
  info[6] = super_used ? 2 : (packed_used ? 1 : 0);
  info[7] = super_used ? super_gathers : 0;
  API_END();
}

int OHXBoosterGetNumGroups(BoosterHandle handle, bst_ulong* out) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  if (out == nullptr) throw OhxError("OHXBoosterGetNumGroups: out is NULL");
  if (!b->loaded) throw OhxError("the booster holds no model: call XGBoosterLoadModel first");
  *out = b->num_groups;
  API_END();
}

int OHXBoosterGetNumCategoricalSplits(BoosterHandle handle, bst_ulong* out) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  if (out == nullptr) throw OhxError("OHXBoosterGetNumCategoricalSplits: out is NULL");
  if (!b->loaded) throw OhxError("the booster holds no model: call XGBoosterLoadModel first");
  *out = b->num_cat;
  API_END();
}

int OHXBoosterKernelSymbol(BoosterHandle handle, bst_ulong ncol, const char** out) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  if (out == nullptr) throw OhxError("OHXBoosterKernelSymbol: out is NULL");
  ensure_uploaded(*b);
  if (b->num_cat != 0) {
    b->symbol = cat_kernel_symbol(b->forest.num_feature, false, b->cat_force_direct);
    *out = b->symbol.c_str();
    return 0;
  }
  b->symbol = predict_kernel_symbol(pick_kernel(*b), device_forest(*b), (uint32_t)ncol, b->tune);
  *out = b->symbol.c_str();
  API_END();
}

int OHXBoosterKernelSymbolRows(BoosterHandle handle, DMatrixHandle dmat, const char** out) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  DMatrixObj* d = as_dmat(dmat);
  if (out == nullptr) throw OhxError("OHXBoosterKernelSymbolRows: out is NULL");
  check_columns(*b, d->ncol);
  ensure_uploaded(*b);
  if (b->num_cat != 0) {
    b->symbol = cat_kernel_symbol(b->forest.num_feature, false, b->cat_force_direct);
    *out = b->symbol.c_str();
    return 0;
  }
  PredictArgs a;
  a.rows = d->d_data;
  a.nrow = d->nrow;
  a.ncol = (uint32_t)d->ncol;
  a.missing = d->missing;
  tree_range(*b, 0, &a.tree_begin, &a.tree_end);
  LaunchTuning tune = tune_for(*b, *d);
  leaf_room(*b, d->nrow, a.tree_end - a.tree_begin, tune, tune.grid_im, tune.grid_jm, tune.grid_row0, /*plan_only=*/true);
  if (d->ncol == 27) (void)defer_plan(*b, d->nrow, tune);
  b->symbol = predict_kernel_symbols_rows(pick_kernel(*b), device_forest(*b), a, b->dev.num_cus, tune);
  *out = b->symbol.c_str();
  API_END();
}

int OHXBoosterRingReruns(BoosterHandle handle, void* stream, bst_ulong* out) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  if (out == nullptr) throw OhxError("OHXBoosterRingReruns: out is NULL");
  *out = 0;
  if (b->uploaded) {
    uint32_t n = 0;
    HIP_CHECK(hipMemcpyAsync(&n, b->d_flags.p + 1, sizeof(n), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
    HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    *out = n;
  }
  API_END();
}

int OHXBoosterCopyEngineChoice(BoosterHandle handle, int* choice, unsigned* trials, unsigned* picked_dma) {
  API_BEGIN();
  BoosterObj* b = as_booster(handle);
  const bool in_charge = g_copy_engine.load(std::memory_order_relaxed) == kCopyAuto && g_host_registry.on.load(std::memory_order_relaxed);
  if (choice) *choice = in_charge ? b->copy_trial.choice : -1;
  if (trials) *trials = b->copy_trial.trials;
  if (picked_dma) *picked_dma = b->copy_trial.picked_dma;
  API_END();
}

int OHXUnregisterHost(const void* array) {
  API_BEGIN();
  if (array != nullptr) (void)g_host_registry.forget(array);
  API_END();
}

int OHXReleaseScratch(void) {
  API_BEGIN();
  g_row_pool.release_all();
  g_host_registry.release_all();
  {
    std::lock_guard<std::mutex> g(g_post.mu);
    for (auto& bf : g_post.buf) bf.release();
  }
  API_END();
}

}  // extern "C"
#pragma GCC visibility pop
