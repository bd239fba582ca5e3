// Private types of libkvgpu's runtime, shared by its three translation units: the pools
// (kvmem.cpp), the device runtime and sessions (kvapi.cpp) and the host-side reading of a fetched
// result (kvresult.cpp). Everything up to the KVRT_DEVICE section compiles without HIP headers
// (kvresult.cpp is also built for the host harness, tools/kvemu); kvmem.cpp and kvapi.cpp define
// KVRT_DEVICE after including <hip/hip_runtime.h>.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kvgpu.h"
#include "kvcond.h"
#include "kvblocks.h"
#include "kvforeach.h"
#include "kvinternal.hpp"
#include "kvjit.hpp"

namespace kvh {

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

int fail(kv_error** err, int code, const std::string& msg);  // fills *err (when given), returns code

// The exception boundary of every C entry point: no exception crosses the ABI. bad_alloc is
// KV_E_NOMEM, a HipError KV_E_DEVICE, any other std::exception the entry point's own code `other`;
// an entry point that takes a kv_error** passes it on.
template <class F>
int guarded(int other, kv_error** err, F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc& e) {
    return fail(err, KV_E_NOMEM, e.what());
  } catch (const HipError& e) {
    return fail(err, KV_E_DEVICE, e.what());
  } catch (const std::exception& e) {
    return fail(err, other, e.what());
  }
}

// a page-locked block from the pinned pool (kvmem.cpp PinnedPool::take / give; null: none to be had)
void* pinned_take(size_t bytes, size_t* cap);
void pinned_give(void* p, size_t cap);

// Host array without value-initialisation; page-locked (pooled hipHostMalloc) unless
// KVGPU_PINNED=0, so device-to-host copies of results are direct DMA.
template <class T>
struct HostArray {
  T* p = nullptr;
  size_t n = 0, cap = 0;
  bool pinned = false;
  HostArray() = default;
  HostArray(const HostArray&) = delete;
  HostArray& operator=(const HostArray&) = delete;
  HostArray(HostArray&& o) noexcept : p(o.p), n(o.n), cap(o.cap), pinned(o.pinned) { o.p = nullptr; o.n = 0; }
  ~HostArray() { release(); }
  void alloc(size_t count) {
    release();
    n = count;
    if (!count) return;
    static const bool use_pinned = !(getenv("KVGPU_PINNED") && getenv("KVGPU_PINNED")[0] == '0');
    if (use_pinned && (p = (T*)pinned_take(count * sizeof(T), &cap)) != nullptr) {
      pinned = true;
      return;
    }
    p = (T*)malloc(count * sizeof(T));
    if (!p) throw std::bad_alloc();
  }
  void release() {
    if (p) {
      if (pinned) pinned_give(p, cap);
      else free(p);
    }
    p = nullptr;
    n = 0;
    cap = 0;
    pinned = false;
  }
  T* data() const { return p; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  T& operator[](size_t i) const { return p[i]; }
};

struct DevPolicySet;  // kvapi.cpp
struct DevBatchRes;

}  // namespace kvh

using namespace kv;
using namespace kvh;

struct kv_policyset {
  PolicySet ps;
  std::unique_ptr<JitImage> jit;  // KV_COMPILE_SPECIALIZE
  std::mutex mu;
  std::map<int, std::unique_ptr<DevPolicySet>> dev;
  kv_policyset();  // (kvapi.cpp, where DevPolicySet is complete)
  ~kv_policyset();
};

struct kv_batch {
  Batch b;
  const kv_policyset* owner = nullptr;
  std::mutex mu;
  // device copies, shared with the sessions that use them (a session keeps its copy alive when
  // the batch drops it: kv_batch_free, a parts session's detach)
  std::map<int, std::shared_ptr<DevBatchRes>> dev;
  std::once_flag dyn_once;
  DynHost dyn;  // pattern-variable tables (build_dyn), on first use
  const DynHost& dyn_host(const PolicySet& ps) {
    std::call_once(dyn_once, [&]() { build_dyn(ps, b, &dyn); });
    return dyn;
  }
  std::once_flag pre_once;
  CondHost pre;  // precondition tables (build_pre), on first use by the host accessors
  const CondHost& pre_host(const PolicySet& ps) {
    std::call_once(pre_once, [&]() { build_pre(ps, b, &pre); });
    return pre;
  }
  std::once_flag fe_once;
  FeHost fe;  // foreach tables (build_foreach), on first use by the host accessors
  const FeHost& fe_host(const PolicySet& ps) {
    std::call_once(fe_once, [&]() { build_foreach(ps, b, &fe); });
    return fe;
  }
  // caller index -> store index (the inverse of Batch::order), on first use; null: identity
  std::once_flag inv_once;
  std::vector<uint32_t> inv;
  const uint32_t* inverse() {
    if (b.order.empty()) return nullptr;
    std::call_once(inv_once, [&]() {
      inv.assign(b.order.size(), 0);
      for (size_t i = 0; i < b.order.size(); i++) inv[b.order[i]] = (uint32_t)i;
    });
    return inv.data();
  }
};

// Records of one device shard: FAIL / ERROR / SKIP pairs, rule-major and in
// resource order (kv_rec_* kernels). Record of (rule, local res): base[rule] +
// offs[rule][tile] + the record pairs before it in its tile (from the statuses).
struct ResultPart {
  std::shared_ptr<kv_batch> shard;  // the shard's batch (null: the result's own batch)
  uint64_t lo = 0, n = 0;           // resources [lo, lo + n) of the result
  uint32_t tiles = 0;
  HostArray<uint32_t> offs;         // [rule][tile] exclusive record offsets within the rule (page-locked:
                                    // C3's 38 MB crossed PCIe through a staging copy at ~1 GB/s)
  std::vector<uint64_t> base;       // [rule + 1] record offsets of the rules
  HostArray<ErrRec8> rec;           // compact records (with `uni`: only the rules that are not uniform)
  HostArray<ErrRec> recw;           // full records, parallel to rec (only when some record is wide)
  // Record codes (kv_rec_code_kernel): record i of a coded rule is its rule's table entry
  // tab[rule * KV_REC_CODES + code[i]] (the lane field left out); a raw rule's records are
  // rec[nbase[rule] ...). Empty `raw`: rec holds every record.
  std::vector<uint8_t> raw;
  std::vector<ErrRec8> tab;
  HostArray<uint8_t> code;
  std::vector<uint64_t> nbase;
  // Status transfer form (kv_status_pack_kernel): the flags of the (rule, KV_RWG-status segment)s
  // the pass wrote, their statuses at 4 bits (KV_RWG / 2 bytes a segment, rule-major), the first
  // packed segment of each rule; the other segments are NOMATCH. Empty sflag: the part's statuses
  // crossed as dense rows of kv_result::status.
  HostArray<uint8_t> sflag, spack;
  std::vector<uint64_t> sbase;
  uint64_t nwg = 0;
  // Pattern sets of foreach rules (KV_COMPILE_FOREACH_PATTERN; fetched with the statuses), in
  // store order: [pattern set][n] the reduction key (kvforeach.h: the deciding element and its
  // code) and the deciding element's 8-byte record
  HostArray<uint32_t> fe_key;
  HostArray<ErrRec8> fe_rec;
  // Rules of several entries (KV_COMPILE_FOREACH_ENTRIES; fetched with the statuses), in store
  // order: [chain][n] the chain key (kvforeach.h kv_fe_chain: the deciding entry, element and code)
  HostArray<uint32_t> fe_ckey;
  // Any sets of foreach rules (KV_COMPILE_FOREACH_ANYPATTERN; fetched with the statuses), in store
  // order: [any set][n] the reduction key and the deciding element's code word (kvforeach.h: 4
  // bits per alternative), [alternative][n] that element's record per alternative (alternatives
  // numbered through the any sets in order)
  HostArray<uint32_t> fe_akey, fe_acode;
  HostArray<ErrRec8> fe_arec;
  // statuses [lo, lo + n) of rule `rule` from the transfer form into dst[0, n)
  void unpack_row(uint32_t rule, uint8_t* dst) const;
  uint64_t n_rec() const { return base.empty() ? 0 : base.back(); }
  // record i of rule `rule` (base[rule] <= i < base[rule + 1])
  ErrRec8 r8(uint32_t rule, uint64_t i) const {
    if (raw.empty()) return rec[i];
    return raw[rule] ? rec[nbase[rule] + (i - base[rule])] : tab[(size_t)rule * KV_REC_CODES + code[i]];
  }
};

struct kv_result {
  const PolicySet* ps = nullptr;  // (host reading needs the compiled set only, not its device side)
  const kv_batch* b = nullptr;
  uint64_t n_rules = 0, n_res = 0;
  // [rule][res] in the batch's store order (Batch::order), or in the caller's order with
  // caller_order; `res` below is an index into it unless named a caller index.
  // kv_result_status returns the caller order (status_c, a host permutation, when they differ).
  HostArray<uint8_t> status;
  std::once_flag sc_once;
  HostArray<uint8_t> status_c;
  // the parts hold their statuses in the transfer form (ResultPart::sflag) until an accessor
  // materialises `status` (st_store) or the caller-order copy (status_caller)
  bool sparse = false;
  std::once_flag st_once;
  // statuses and records were fetched in the caller's order (a permuted batch fetched whole:
  // DevSession::fetch); `status` is then the caller order and `res` below a caller index
  bool caller_order = false;
  std::vector<ResultPart> parts;    // by resource range
  bool errors = false;              // KV_MODE_ERRORS: records fetched
  std::vector<int64_t> counts;
  std::vector<int64_t> scope_counts;  // [scope][rule][KV_HIST] (KV_MODE_SCOPES)
  double kernel_ms = 0;
  uint32_t mode = 0;
  // wall-clock phases of the kv_validate that made this result (kv_result_phase): upload, setup,
  // pass, then the fetch's device work and copies, each ended by a stream synchronize
  std::vector<std::pair<std::string, double>> phases;
  // bulk failure export (kv_result_failures), built on first use
  std::once_flag fail_once;
  std::vector<uint32_t> f_rule, f_path;
  std::vector<uint64_t> f_res;
  std::vector<std::string> f_paths;

  bool has_err() const { return errors; }
  // store index of caller index `res`
  uint64_t sidx(uint64_t res) const { return caller_order ? res : store_of(res); }
  // the batch's store slot of caller index `res` (indexes the batch-side tables: dynamic leaves)
  uint64_t store_of(uint64_t res) const {
    const uint32_t* iv = const_cast<kv_batch*>(b)->inverse();
    return iv ? iv[res] : res;
  }
  // caller index of status / record index `s`
  uint64_t cidx(uint64_t s) const { return caller_order || b->b.order.empty() ? s : b->b.order[s]; }
  bool has_status() const { return sparse || !status.empty(); }
  static unsigned host_threads() { return std::max(1u, std::min<unsigned>(16u, std::thread::hardware_concurrency())); }
  // out[c] = row[inv[c]] (a gather: sequential 8-byte stores, reads from a row that stays in the
  // core's cache; 2.5x the rate of the scatter out[ord[q]] = row[q] on this host's cores)
  static void gather_row(const uint8_t* row, const uint32_t* inv, uint64_t n, uint8_t* out);
  // rows [rule][0, n_res) of dst from the parts' transfer form, rules split over host threads;
  // with `inv` (caller index -> store index) each row is unpacked in store order and gathered
  void unpack_rows(uint8_t* dst, const uint32_t* inv) const;
  // the status matrix in the records' order (store order unless caller_order), materialised from
  // the transfer form on first use
  const uint8_t* st_store();
  // the statuses in caller order: rows of the store-order matrix gathered through the batch's
  // inverse order, rules split over host threads (a permuted batch only); from the transfer form directly
  // when the store-order matrix was not materialised
  const uint8_t* status_caller();
  const Batch& batch_of(const ResultPart& p) const { return p.shard ? p.shard->b : b->b; }
  const ResultPart* part_of(uint64_t res) const {
    for (const ResultPart& p : parts)
      if (res >= p.lo && res < p.lo + p.n) return &p;
    return nullptr;
  }
  static ErrRec decode(const ErrRec8& c);
  // record index of pair (rule, res) within its part
  uint64_t rec_index(const ResultPart& p, uint32_t rule, uint64_t res) const;
  // error record of a FAIL / ERROR / SKIP pair, and the batch its node ids refer to
  bool err(uint32_t rule, uint64_t res, ErrRec* e, const Batch** bt) const;
};

#ifdef KVRT_DEVICE  // ---- the device side (kvmem.cpp, kvapi.cpp)
#include <tuple>

#define HIPCHK(x)                                                                              \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) throw HipError(std::string(#x) + ": " + hipGetErrorString(e_));      \
  } while (0)

namespace kvh {

bool pinned_src(const void* src, size_t bytes);  // page-locked store array (PinnedStore)
size_t dev_pool_held(int device);                // bytes of released device buffers kept (DevPool)

// Idle HIP streams per (device, flags, priority) and every stream ever created per device (kvmem.cpp)
struct StreamPool {
  std::mutex mu;
  std::map<std::tuple<int, unsigned, int>, std::vector<hipStream_t>> free;
  std::map<int, std::vector<hipStream_t>> all;
  static StreamPool& get();
  std::vector<hipStream_t> streams_of(int dev);
  // a stream of the current device `dev`; low: the lowest scheduling priority (its workgroups are
  // dispatched when the other queues' kernels leave slots free)
  hipStream_t take(int dev, unsigned flags, bool low = false);
  void give(int dev, unsigned flags, hipStream_t s, bool low = false);
  static int lowest();
};

// A device buffer from the device pool (kvmem.cpp DevPool)
struct DevBuf {
  void* p = nullptr;
  size_t n = 0, cap = 0;
  int dev = -1;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  template <class T, class A>
  void upload(const std::vector<T, A>& v, int device) {
    upload_raw(v.data(), v.size() * sizeof(T), device);
  }
  void upload_raw(const void* src, size_t bytes, int device) {
    alloc(bytes, device);
    if (bytes) upload_h2d(p, src, bytes);
  }
  // a page-locked source is copied asynchronously on `st` (the caller synchronizes `st` before
  // the source may change or the buffer is read elsewhere); a pageable one as upload_raw
  template <class T, class A>
  void upload_async(const std::vector<T, A>& v, int device, hipStream_t st) {
    const size_t bytes = v.size() * sizeof(T);
    alloc(bytes, device);
    if (!bytes) return;
    if (pinned_src(v.data(), bytes))
      HIPCHK(hipMemcpyAsync(p, v.data(), bytes, hipMemcpyHostToDevice, st));
    else
      upload_h2d(p, v.data(), bytes);
  }
  static void upload_h2d(void* dst, const void* src, size_t bytes);
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(n, o.n);
    std::swap(cap, o.cap);
    std::swap(dev, o.dev);
  }
  void alloc(size_t bytes, int device);  // (a buffer allocated before is released first)
  void release();
};

}  // namespace kvh
#endif  // KVRT_DEVICE
