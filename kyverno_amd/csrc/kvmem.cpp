// The pools of libkvgpu's device runtime: HIP streams, device buffers, page-locked host blocks
// (result arrays, the store arrays of ingested batches) and DevBuf's upload paths.
#include <hip/hip_runtime.h>

#include <cstring>
#define KVRT_DEVICE 1
#include "kvrt.hpp"

namespace kvh {

// HIP streams cost milliseconds to create and to destroy on this runtime (hipStreamCreate* 2.3-3.8
// ms, hipStreamDestroy 1.8-2.6 ms per call in the rocprofv3 HIP API trace of a C2 kv_validate: 15 of
// its 44 ms), so sessions and staged uploads take idle streams from a per-(device, flags) pool and
// give them back instead. The pool also knows every stream it ever created per device (`all`): a
// released device buffer becomes reusable once an event recorded on each of them has completed
// (DevPool below).
StreamPool& StreamPool::get() {
  static StreamPool* p = new StreamPool();  // never destroyed (streams die with the process)
  return *p;
}
std::vector<hipStream_t> StreamPool::streams_of(int dev) {
  std::lock_guard<std::mutex> g(mu);
  return all[dev];
}
hipStream_t StreamPool::take(int dev, unsigned flags, bool low) {
  const int prio = low ? lowest() : 0;
  {
    std::lock_guard<std::mutex> g(mu);
    auto& v = free[{dev, flags, prio}];
    if (!v.empty()) {
      hipStream_t s = v.back();
      v.pop_back();
      return s;
    }
  }
  hipStream_t s = nullptr;
  if (low) HIPCHK(hipStreamCreateWithPriority(&s, flags, prio));
  else HIPCHK(hipStreamCreateWithFlags(&s, flags));
  std::lock_guard<std::mutex> g(mu);
  all[dev].push_back(s);
  return s;
}
void StreamPool::give(int dev, unsigned flags, hipStream_t s, bool low) {
  if (!s) return;
  (void)hipStreamSynchronize(s);
  const int prio = low ? lowest() : 0;
  std::lock_guard<std::mutex> g(mu);
  free[{dev, flags, prio}].push_back(s);
}
int StreamPool::lowest() {
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return least;
}

// Device allocations are expensive to create and to free (hipMalloc maps pages, hipFree also
// waits for the device), and a host that validates batch after batch allocates the same store,
// column and result buffers for every batch. Released buffers are therefore kept per device and
// handed to the next allocation of a similar size. A released block is reusable once the work
// queued before its release has finished (hipFree's own guarantee, without blocking the releasing
// thread or any other session on the device): give() records an event on every stream the library
// created on the device and on the null stream, and take() hands the block out only when all of
// them have completed. At most kv_device_pool_limit() bytes are kept (default 32 GiB of the 288 GiB
// HBM); when a hipMalloc fails the device's kept buffers are freed and the allocation retried, and
// kv_device_trim() returns them to the device for co-resident allocators (e.g. torch).
// KVGPU_DEVPOOL=0: plain hipMalloc / hipFree.
struct DevPool {
  struct Pending {
    void* p;
    size_t cap;
    std::vector<hipEvent_t> ev;
  };
  std::mutex mu;
  std::map<int, std::multimap<size_t, void*>> free;  // device -> capacity -> block
  std::map<int, std::vector<Pending>> pending;        // released, maybe still in use by queued work
  std::map<int, size_t> held;                         // free + pending bytes
  std::map<int, std::vector<hipEvent_t>> evs;         // idle events per device
  size_t hold = 32ull << 30;
  static DevPool& get() {
    static DevPool* p = new DevPool();  // never destroyed: buffers may be released during static teardown
    return *p;
  }
  static bool enabled() {
    static const bool on = !(getenv("KVGPU_DEVPOOL") && getenv("KVGPU_DEVPOOL")[0] == '0');
    return on;
  }
  // (mu held) pending blocks whose events have all completed move to the free list
  void settle(int dev) {
    auto& pv = pending[dev];
    for (size_t i = 0; i < pv.size();) {
      bool done = true;
      for (hipEvent_t e : pv[i].ev) {
        const hipError_t q = hipEventQuery(e);
        if (q == hipErrorNotReady) {
          done = false;
          break;
        }
        if (q != hipSuccess) (void)hipGetLastError();
      }
      if (!done) {
        i++;
        continue;
      }
      for (hipEvent_t e : pv[i].ev) evs[dev].push_back(e);
      free[dev].emplace(pv[i].cap, pv[i].p);
      pv[i] = std::move(pv.back());
      pv.pop_back();
    }
  }
  // a block of at least `bytes` on the current device `dev` (its capacity in *cap)
  void* take(int dev, size_t bytes, size_t* cap) {
    if (enabled()) {
      std::lock_guard<std::mutex> g(mu);
      settle(dev);
      auto& f = free[dev];
      auto it = f.lower_bound(bytes);
      if (it != f.end() && it->first <= bytes + bytes / 4 + (2u << 20)) {
        void* p = it->second;
        *cap = it->first;
        held[dev] -= it->first;
        f.erase(it);
        return p;
      }
    }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      trim(dev);
      HIPCHK(hipMalloc(&p, bytes));
    }
    *cap = bytes;
    return p;
  }
  // `dev` is the current device
  void give(int dev, void* p, size_t cap) {
    if (enabled()) {
      std::vector<hipStream_t> st = StreamPool::get().streams_of(dev);
      st.push_back(nullptr);  // (the null stream: synchronous copies, RCCL setup)
      std::lock_guard<std::mutex> g(mu);
      if (held[dev] + cap <= hold) {
        Pending pe{p, cap, {}};
        bool ok = true;
        for (hipStream_t s : st) {
          hipEvent_t e = nullptr;
          auto& idle = evs[dev];
          if (!idle.empty()) {
            e = idle.back();
            idle.pop_back();
          } else if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            ok = false;
            break;
          }
          pe.ev.push_back(e);
          if (hipEventRecord(e, s) != hipSuccess) {
            (void)hipGetLastError();
            ok = false;
            break;
          }
        }
        if (ok) {
          pending[dev].push_back(std::move(pe));
          held[dev] += cap;
          return;
        }
        for (hipEvent_t e : pe.ev) evs[dev].push_back(e);
      }
    }
    (void)hipDeviceSynchronize();  // (hipFree waits for the device anyway)
    (void)hipFree(p);
  }
  size_t held_on(int dev) {
    std::lock_guard<std::mutex> g(mu);
    return held[dev];
  }
  // free every kept block of `dev` (the current device): waits for the device first
  void trim(int dev) {
    std::multimap<size_t, void*> f;
    std::vector<Pending> pv;
    {
      std::lock_guard<std::mutex> g(mu);
      f.swap(free[dev]);
      pv.swap(pending[dev]);
      held[dev] = 0;
    }
    if (f.empty() && pv.empty()) return;
    (void)hipDeviceSynchronize();
    for (auto& [c, p] : f) (void)hipFree(p);
    std::lock_guard<std::mutex> g(mu);
    for (Pending& pe : pv) {
      (void)hipFree(pe.p);
      for (hipEvent_t e : pe.ev) evs[dev].push_back(e);
    }
  }
};

size_t dev_pool_held(int device) { return DevPool::get().held_on(device); }

// Host-to-device copy of a (pageable) host range. Large ranges go through a pinned staging
// ring: host threads copy chunk i into a page-locked buffer while the DMA engine moves chunk
// i-1 (32 MB chunks, 4 buffers, up to 16 copy threads).
void DevBuf::upload_h2d(void* dst, const void* src, size_t bytes) {
  constexpr size_t kChunk = 32u << 20;
  constexpr size_t kMin = 16u << 20;
  constexpr int kRing = 4;
  if (bytes < kMin || pinned_src(src, bytes)) {
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return;
  }
  static std::mutex mu;  // one staged upload at a time per process (the ring is shared)
  static char* ring[kRing] = {};
  std::lock_guard<std::mutex> g(mu);
  if (!ring[0]) {
    for (int i = 0; i < kRing; i++) {
      if (hipHostMalloc((void**)&ring[i], kChunk, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        for (int j = 0; j < i; j++) (void)hipHostFree(ring[j]);
        ring[0] = nullptr;
        HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return;
      }
    }
  }
  int sdev = 0;
  HIPCHK(hipGetDevice(&sdev));
  hipStream_t st = StreamPool::get().take(sdev, hipStreamNonBlocking);
  hipEvent_t ev[kRing];
  for (int i = 0; i < kRing; i++) HIPCHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
  bool used[kRing] = {};
  static const unsigned T = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  size_t k = 0;
  for (size_t off = 0; off < bytes; off += kChunk, k++) {
    const int i = (int)(k % kRing);
    const size_t len = std::min(kChunk, bytes - off);
    if (used[i]) HIPCHK(hipEventSynchronize(ev[i]));  // the DMA out of this buffer is done
    const char* s = (const char*)src + off;
    std::vector<std::thread> th;
    const size_t part = (len + T - 1) / T;
    for (unsigned t = 0; t < T; t++) {
      const size_t a = std::min(len, t * part), e = std::min(len, a + part);
      if (a < e) th.emplace_back([=]() { memcpy(ring[i] + a, s + a, e - a); });
    }
    for (auto& x : th) x.join();
    HIPCHK(hipMemcpyAsync((char*)dst + off, ring[i], len, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ev[i], st));
    used[i] = true;
  }
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < kRing; i++) (void)hipEventDestroy(ev[i]);
  StreamPool::get().give(sdev, hipStreamNonBlocking, st);
}
void DevBuf::alloc(size_t bytes, int device) {
  release();
  dev = device;
  n = bytes;
  p = DevPool::get().take(device, std::max<size_t>(bytes, 16), &cap);
}
void DevBuf::release() {
  if (!p) return;
  int cur;
  if (hipGetDevice(&cur) == hipSuccess) {
    (void)hipSetDevice(dev);
    DevPool::get().give(dev, p, cap);
    (void)hipSetDevice(cur);
  }
  p = nullptr;
  n = 0;
  cap = 0;
}

// Page-locked host blocks are expensive to create (pinning), so released result
// buffers are kept for the next result of the process (up to 8 GiB): a host that
// validates batch after batch pays the pinning once.
// A caller that knows its batches' size can page-lock an arena up front (kv_host_reserve, outside
// ingest): blocks are then carved from it (first fit, 2 MiB granules, freed ranges coalesce) before
// any new block is page-locked, so even a process's first batch ingests into page-locked memory
// that is already there.
struct PinnedPool {
  std::mutex mu;
  std::multimap<size_t, void*> free;  // capacity -> block
  size_t held = 0;
  char* arena = nullptr;
  size_t arena_bytes = 0;
  std::map<size_t, size_t> arena_free;  // offset -> bytes
  static constexpr size_t kGran = 2u << 20;
  static PinnedPool& get() {
    static PinnedPool* p = new PinnedPool();  // never destroyed: blocks may outlive static teardown
    return *p;
  }
  bool reserve(size_t bytes) {
    std::lock_guard<std::mutex> g(mu);
    if (arena) return arena_bytes >= bytes;
    bytes = (bytes + kGran - 1) / kGran * kGran;
    void* p = nullptr;
    if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    arena = (char*)p;
    arena_bytes = bytes;
    arena_free[0] = bytes;
    return true;
  }
  bool in_arena(const void* p) const { return arena && (const char*)p >= arena && (const char*)p < arena + arena_bytes; }
  void* take(size_t bytes, size_t* cap) {
    {
      std::lock_guard<std::mutex> g(mu);
      auto it = free.lower_bound(bytes);
      if (it != free.end() && it->first <= 2 * bytes + (1u << 20)) {
        void* p = it->second;
        *cap = it->first;
        held -= it->first;
        free.erase(it);
        return p;
      }
      if (arena) {
        const size_t want = (bytes + kGran - 1) / kGran * kGran;
        for (auto a = arena_free.begin(); a != arena_free.end(); ++a)
          if (a->second >= want) {
            const size_t off = a->first, left = a->second - want;
            arena_free.erase(a);
            if (left) arena_free[off + want] = left;
            *cap = want;
            return arena + off;
          }
      }
    }
    // headroom (+1/8, 16 MiB granules) so the next batch's slightly larger result fits the block
    const size_t want = bytes < (16u << 20) ? bytes : ((bytes + bytes / 8 + (16u << 20) - 1) & ~(size_t)((16u << 20) - 1));
    void* p = nullptr;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    *cap = want;
    return p;
  }
  void give(void* p, size_t cap) {
    std::lock_guard<std::mutex> g(mu);
    if (in_arena(p)) {  // back into the arena, merged with its free neighbours
      size_t off = (size_t)((char*)p - arena), len = cap;
      auto nx = arena_free.lower_bound(off);
      if (nx != arena_free.end() && nx->first == off + len) {
        len += nx->second;
        nx = arena_free.erase(nx);
      }
      if (nx != arena_free.begin()) {
        auto pv = std::prev(nx);
        if (pv->first + pv->second == off) {
          off = pv->first;
          len += pv->second;
          arena_free.erase(pv);
        }
      }
      arena_free[off] = len;
      return;
    }
    if (held + cap > (8ull << 30)) {
      (void)hipHostFree(p);
      return;
    }
    free.emplace(cap, p);
    held += cap;
  }
};

// Page-locked store arrays of ingested batches (kvinternal.hpp HostMem): blocks from the
// pool, registered by address so the upload can tell a page-locked source (direct DMA)
// from a pageable one (staging ring), and so a block returns to the pool when freed.
struct PinnedStore {
  std::mutex mu;
  std::map<uintptr_t, size_t> live;  // block -> capacity
  static PinnedStore& get() {
    static PinnedStore* p = new PinnedStore();
    return *p;
  }
  static bool enabled() {
    static const bool on = []() {
      if (getenv("KVGPU_PINNED") && getenv("KVGPU_PINNED")[0] == '0') return false;
      int n = 0;  // no device (host-only use of the library): plain memory
      if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return false;
      }
      return true;
    }();
    return on;
  }
  static void* take(size_t bytes) {
    if (!enabled()) return nullptr;
    size_t cap = 0;
    void* p = PinnedPool::get().take(bytes, &cap);
    if (!p) return nullptr;
    std::lock_guard<std::mutex> g(get().mu);
    get().live[(uintptr_t)p] = cap;
    return p;
  }
  static bool give(void* p) {
    size_t cap = 0;
    {
      std::lock_guard<std::mutex> g(get().mu);
      auto it = get().live.find((uintptr_t)p);
      if (it == get().live.end()) return false;
      cap = it->second;
      get().live.erase(it);
    }
    PinnedPool::get().give(p, cap);
    return true;
  }
  // [src, src + bytes) inside one live page-locked block
  static bool contains(const void* src, size_t bytes) {
    std::lock_guard<std::mutex> g(get().mu);
    auto& m = get().live;
    auto it = m.upper_bound((uintptr_t)src);
    if (it == m.begin()) return false;
    --it;
    return (uintptr_t)src + bytes <= it->first + it->second;
  }
};
struct InstallHostMem {
  InstallHostMem() {
    g_hostmem.take = &PinnedStore::take;
    g_hostmem.give = &PinnedStore::give;
  }
} install_host_mem_;

bool pinned_src(const void* src, size_t bytes) { return PinnedStore::contains(src, bytes); }
void* pinned_take(size_t bytes, size_t* cap) { return PinnedPool::get().take(bytes, cap); }
void pinned_give(void* p, size_t cap) { PinnedPool::get().give(p, cap); }

}  // namespace kvh

extern "C" {

int kv_host_reserve(uint64_t bytes) {
  return guarded(KV_E_DEVICE, nullptr,
                 [&]() { return PinnedStore::enabled() && PinnedPool::get().reserve(bytes) ? 0 : KV_E_DEVICE; });
}

int kv_device_pool_limit(uint64_t bytes) {
  DevPool& p = DevPool::get();
  std::lock_guard<std::mutex> g(p.mu);
  p.hold = (size_t)bytes;
  return 0;
}

int kv_device_trim(int device) {
  int n = 0, cur = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n || hipGetDevice(&cur) != hipSuccess) {
    (void)hipGetLastError();
    return KV_E_DEVICE;
  }
  if (hipSetDevice(device) != hipSuccess) {
    (void)hipGetLastError();
    return KV_E_DEVICE;
  }
  DevPool::get().trim(device);
  (void)hipSetDevice(cur);
  return 0;
}

}  // extern "C"
