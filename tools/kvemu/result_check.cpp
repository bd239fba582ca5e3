// result_check: the host-side reading of a fetched result (kyverno_amd/csrc/kvresult.cpp) under
// ASan/UBSan, without a device. Test infrastructure only (tests/test_result_cpu.py).
//
//   result_check <policies.json> <resources.json> <compile flags> <status.u8>
//
// compiles and ingests as libkvgpu does, then builds kv_results by hand from the given status
// matrix ([rule][res], the caller's order) in the forms a fetch produces: the dense matrix in store
// order, the packed transfer form (sflag / spack / sbase) and the caller's order, as one part and as
// three shard parts. Records are not built. Prints one JSON object: the batch's store order and,
// per form, the st_store() and status_caller() matrices and every non-zero answer of the per-pair
// message accessors ([rule, res, text or negative code]; foreach_element: the index).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../kyverno_amd/csrc/kvrt.hpp"

// the result arrays' page-locked blocks: plain memory here (exact sizes, so ASan sees every overrun)
void* kvh::pinned_take(size_t bytes, size_t* cap) {
  *cap = bytes;
  return malloc(bytes);
}
void kvh::pinned_give(void* p, size_t) { free(p); }

namespace {

std::string slurp(const char* p) {
  std::ifstream f(p, std::ios::binary);
  if (!f) throw std::runtime_error(std::string("cannot read ") + p);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

std::string quoted(const std::string& s) {
  std::string o = "\"";
  char u[8];
  for (unsigned char c : s) {
    if (c == '"' || c == '\\') (o += '\\') += (char)c;
    else if (c < 0x20) snprintf(u, sizeof u, "\\u%04x", c), o += u;
    else o += (char)c;
  }
  return o + "\"";
}

// statuses [0, n) of every rule (row stride `stride`) as kv_status_pack_kernel leaves them: a flag
// per (rule, KV_RWG-status segment) with a status other than NOMATCH, those segments at 4 bits a status
void pack(const uint8_t* st, uint64_t stride, uint64_t n_rules, ResultPart* p) {
  p->nwg = (p->n + KV_RWG - 1) / KV_RWG;
  p->sbase.assign(n_rules, 0);
  p->sflag.alloc(n_rules * p->nwg);
  std::vector<uint8_t> bytes;
  for (uint64_t r = 0; r < n_rules; r++) {
    p->sbase[r] = bytes.size() / (KV_RWG / 2);
    for (uint64_t g = 0; g < p->nwg; g++) {
      const uint8_t* seg = st + r * stride + g * KV_RWG;
      const uint64_t m = std::min<uint64_t>(KV_RWG, p->n - g * KV_RWG);
      bool any = false;
      for (uint64_t i = 0; i < m; i++) any |= seg[i] != ST_NOMATCH;
      p->sflag[r * p->nwg + g] = any;
      if (!any) continue;
      const size_t o = bytes.size();
      bytes.resize(o + KV_RWG / 2, 0);
      for (uint64_t i = 0; i < m; i++) bytes[o + i / 2] |= (uint8_t)(seg[i] << (4 * (i & 1)));
    }
  }
  p->spack.alloc(bytes.size());
  if (!bytes.empty()) memcpy(p->spack.data(), bytes.data(), bytes.size());
}

void print_matrix(const char* name, const uint8_t* m, uint64_t n_rules, uint64_t n) {
  printf("\"%s\":[", name);
  for (uint64_t r = 0; r < n_rules; r++) {
    printf("%s[", r ? "," : "");
    for (uint64_t k = 0; k < n; k++) printf(k ? ",%u" : "%u", m[r * n + k]);
    printf("]");
  }
  printf("],");
}

typedef int (*text_fn)(const kv_result*, uint32_t, uint64_t, char*, size_t);

void print_texts(const char* name, text_fn fn, const kv_result& r) {
  printf("\"%s\":[", name);
  bool first = true;
  for (uint32_t rule = 0; rule < r.n_rules; rule++)
    for (uint64_t k = 0; k < r.n_res; k++) {
      const int n = fn(&r, rule, k, nullptr, 0);  // (size, then fill: both calls under the sanitizers)
      if (!n) continue;
      std::string v = std::to_string(n);
      if (n > 0) {
        std::vector<char> buf((size_t)n + 1);
        if (fn(&r, rule, k, buf.data(), buf.size()) != n) throw std::runtime_error("accessor length changed");
        v = quoted(std::string(buf.data(), (size_t)n));
      }
      printf("%s[%u,%llu,%s]", first ? "" : ",", rule, (unsigned long long)k, v.c_str());
      first = false;
    }
  printf("],");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: result_check policies.json resources.json flags status.u8\n");
    return 2;
  }
  try {
    const std::string pol = slurp(argv[1]), res = slurp(argv[2]), in = slurp(argv[4]);
    PolicySet ps;
    compile_policies(pol.data(), pol.size(), &ps, (uint32_t)atoi(argv[3]));
    kv_batch whole;
    ingest_resources(ps, res.data(), res.size(), nullptr, &whole.b);
    const uint64_t R = ps.rules.size(), n = whole.b.res.size();
    if (in.size() != R * n) throw std::runtime_error("status matrix is not [rules][resources]");
    const uint8_t* caller = (const uint8_t*)in.data();
    const std::vector<uint32_t>& order = whole.b.order;  // store index -> caller index (empty: identity)
    // (the index arithmetic under test is the identity on a store that ingest did not permute)
    if (n > 1 && order.empty()) throw std::runtime_error("the batch's store is not permuted: vary the namespaces");
    std::vector<uint8_t> store(R * n);
    for (uint64_t r = 0; r < R; r++)
      for (uint64_t s = 0; s < n; s++) store[r * n + s] = caller[r * n + (order.empty() ? s : order[s])];
    printf("{\"n_rules\":%llu,\"n_res\":%llu,\"order\":[", (unsigned long long)R, (unsigned long long)n);
    for (size_t s = 0; s < order.size(); s++) printf(s ? ",%u" : "%u", order[s]);
    printf("],\"forms\":[");
    bool first = true;
    for (uint32_t G : {1u, 3u})
      for (const char* form : {"dense", "packed", "packed_sc", "caller"}) {
        // (packed_sc: status_caller() before anything materialises the store-order matrix)
        const bool sc_first = !strcmp(form, "packed_sc"), packed = sc_first || !strcmp(form, "packed");
        const bool by_caller = !strcmp(form, "caller");
        if (by_caller && (G != 1 || order.empty())) continue;  // (only a permuted batch fetched whole)
        kv_result r;
        r.ps = &ps;
        r.b = &whole;
        r.n_rules = R;
        r.n_res = n;
        r.sparse = packed;
        r.caller_order = by_caller;
        const uint8_t* src = by_caller ? caller : store.data();
        if (!packed) {
          r.status.alloc(R * n);
          if (R * n) memcpy(r.status.data(), src, R * n);
        }
        for (const auto& rg : shard_ranges(n, G)) {
          r.parts.emplace_back();
          ResultPart& p = r.parts.back();
          p.lo = rg.first;
          p.n = rg.second - rg.first;
          if (G > 1) {
            p.shard = std::make_shared<kv_batch>();
            make_shard(whole.b, rg.first, rg.second, &p.shard->b);
          }
          if (packed) pack(src + p.lo, n, R, &p);
        }
        printf("%s{\"name\":\"%s%u\",\"order\":\"%s\",", first ? "" : ",", form, G, by_caller ? "caller" : "store");
        first = false;
        const uint8_t* sc = nullptr;
        if (sc_first && kv_result_status(&r, &sc, nullptr, nullptr) != 0) throw std::runtime_error("kv_result_status failed");
        // (else the accessors first: on a packed result the first of them materialises the matrix)
        print_texts("subst_error", kv_result_subst_error, r);
        print_texts("precond_message", kv_result_precond_message, r);
        print_texts("deny_message", kv_result_deny_message, r);
        print_texts("foreach_message", kv_result_foreach_message, r);
        printf("\"foreach_element\":[");
        bool f1 = true;
        for (uint32_t rule = 0; rule < R; rule++)
          for (uint64_t k = 0; k < n; k++) {
            uint32_t e = 0;
            const int rc = kv_result_foreach_element(&r, rule, k, &e);
            if (!rc && e == 0xFFFFFFFFu) continue;
            printf("%s[%u,%llu,%lld]", f1 ? "" : ",", rule, (unsigned long long)k, rc ? (long long)rc : (long long)e);
            f1 = false;
          }
        printf("],");
        print_matrix("st_store", r.st_store(), R, n);
        if (kv_result_status(&r, &sc, nullptr, nullptr) != 0) throw std::runtime_error("kv_result_status failed");
        print_matrix("status_caller", sc, R, n);
        printf("\"parts\":%zu}", r.parts.size());
      }
    printf("]}\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "result_check: %s\n", e.what());
    return 1;
  }
}
