// kvemu driver: runs the generated specialized kernels (kvjitgen.cpp output for one
// policy set, compiled for the host with shim.h) over an ingested batch, lane by
// lane, and writes the status matrix and error records. Test / debugging
// infrastructure only (sanitizer runs of the generated code, CPU-side checks of
// the generator against the oracle); the product path is libkvgpu on a GPU.
//
//   kvemu <policies.json> <resources.ndjson> <ctx.json|-> <out-prefix>
//     -> <out-prefix>.status  u8 [rule][res]
//        <out-prefix>.err     ErrRec (32 B) [rule][res], records of FAIL/ERROR/SKIP pairs
//        <out-prefix>.meta    "n_rules n_res wide"
// Environment: the KVGPU_JIT_* settings the source was generated with.
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../kyverno_amd/csrc/kv_layout.h"
#include "../../kyverno_amd/csrc/kvdevtypes.h"
#include "../../kyverno_amd/csrc/kvinternal.hpp"
#include "../../kyverno_amd/csrc/kvjit.hpp"
#include "../../kyverno_amd/csrc/kvcond.h"
#include "../../kyverno_amd/csrc/kvblocks.h"
#include "../../kyverno_amd/csrc/kvforeach.h"

using namespace kv;
using namespace kvh;

struct kvemu_dim3 {
  uint32_t x, y, z;
};
thread_local kvemu_dim3 threadIdx, blockIdx, gridDim;

extern "C" void kvemu_mtab(const DevPS* P, const DevBatch* B, uint32_t words, uint32_t max_entities, uint32_t* ns,
                           uint32_t* an, uint32_t* sl);

std::vector<uint32_t> kvemu_pcol(const DevBatch* B, const std::vector<ColDesc>& cols, const std::vector<uint32_t>& fam_arr,
                                 const std::vector<uint32_t>& fam_parent, const std::vector<uint32_t>& fam_ncols, const std::vector<uint32_t>& fam_nw,
                                 const std::vector<uint32_t>& fam_nb, const std::vector<uint32_t>& fam_nn,
                                 std::vector<uint32_t>* erow);
typedef void (*ptab_fn)(const DevPS*, const Val*, const uint8_t*, uint32_t, uint32_t*);
extern "C" void kvemu_mfac(const DevPS* P, const DevBatch* B, uint32_t* mtup);
// the pattern sets' rows of the foreach plane (fepat.cpp: kvwalk.h as a one-lane wave)
extern "C" void kvemu_foreach_pat(const FeTables* T, const FePatTables* Q, const DevPS* P, const DevBatch* B,
                                  uint32_t n_res, uint8_t* fe_st, const FeVarTables* V, uint32_t n_vpats);
// ... and the any sets' (KV_COMPILE_FOREACH_ANYPATTERN)
extern "C" void kvemu_foreach_any(const FeTables* T, const FeAnyTables* A, const DevPS* P, const DevBatch* B,
                                  uint32_t n_res, uint8_t* fe_st, const FeVarTables* V, uint32_t n_vanys, uint32_t n_pats);
typedef void (*chunk_fn)(const DevPS*, const DevBatch*, const Node*, const Val*, const uint8_t*, DevOut, uint32_t);

static std::string slurp(const char* p) {
  std::ifstream f(p, std::ios::binary);
  if (!f) throw std::runtime_error(std::string("cannot read ") + p);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

static uint64_t fnv1a(const std::string& s) {
  uint64_t h = 1469598103934665603ull;
  for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
  return h;
}

#ifndef KVEMU_SRC_HASH
#define KVEMU_SRC_HASH 0
#endif

// every (block, lane) of a grid, blocks spread over host threads
template <class F>
static void grid(uint32_t bx, uint32_t by, F f, uint32_t lanes = (uint32_t)KV_WG) {
  const uint32_t T = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
  std::atomic<uint64_t> next{0};
  const uint64_t total = (uint64_t)bx * by;
  std::vector<std::thread> th;
  for (uint32_t t = 0; t < T; t++)
    th.emplace_back([&]() {
      for (uint64_t i; (i = next++) < total;) {
        blockIdx = {(uint32_t)(i % bx), (uint32_t)(i / bx), 0};
        gridDim = {bx, by, 1};
        for (uint32_t x = 0; x < lanes; x++) {
          threadIdx = {x, 0, 0};
          f();
        }
      }
    });
  for (auto& t : th) t.join();
}

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: kvemu policies.json resources.ndjson ctx.json|- out-prefix\n");
    return 2;
  }
  try {
    const std::string pol = slurp(argv[1]), res = slurp(argv[2]);
    std::string ctx = strcmp(argv[3], "-") ? slurp(argv[3]) : std::string();
    PolicySet ps;
    // KVEMU_COMPILE_FLAGS: kv_compile's flags (2: KV_COMPILE_DENY, 4: KV_COMPILE_FOREACH, 8:
    // KV_COMPILE_FOREACH_PATTERN, 16: KV_COMPILE_FOREACH_ENTRIES, 32: KV_COMPILE_FOREACH_ANYPATTERN,
    // 64: KV_COMPILE_FOREACH_PATVARS), as the binary's source was generated
    compile_policies(pol.data(), pol.size(), &ps, getenv("KVEMU_COMPILE_FLAGS") ? (uint32_t)atoi(getenv("KVEMU_COMPILE_FLAGS")) : 0u);
    Batch whole;
    ingest_resources(ps, res.data(), res.size(), nullptr, &whole);
    // KVEMU_SHARDS=G: evaluate G contiguous shards (kvshard.cpp, as kv_validate_devices does)
    // one after the other and assemble the statuses in resource order
    const uint32_t G = getenv("KVEMU_SHARDS") ? (uint32_t)std::max(1, atoi(getenv("KVEMU_SHARDS"))) : 1u;
    const auto ranges = shard_ranges(whole.res.size(), G);
    const uint64_t n_total = whole.res.size();
    const std::vector<uint32_t> order = whole.order;  // store order (whole is moved below)
    std::vector<uint8_t> status_all(ps.rules.size() * n_total, 0xEE);
    std::vector<ErrRec> err_all;
    bool wide_any = false;
    const bool want_err_all = !getenv("KVEMU_NO_ERR");
    if (want_err_all) err_all.assign(ps.rules.size() * n_total, ErrRec{});
    for (uint32_t sh = 0; sh < G; sh++) {
    Batch b;
    if (G == 1) b = std::move(whole);
    else make_shard(whole, ranges[sh].first, ranges[sh].second, &b);
    const uint64_t lo = ranges[sh].first;
    JitImage img;
    jit_generate(ps, jit_chunk_rules(), &img);
    if (KVEMU_SRC_HASH && fnv1a(img.source) != (uint64_t)KVEMU_SRC_HASH)
      throw std::runtime_error("generated source differs from the one this binary was built from");

    const std::vector<uint32_t> fflags = fold_filters(ps, ctx.empty() ? nullptr : ctx.c_str());
    std::vector<uint32_t> koff, klen;
    std::string ks;
    key_table(ps, b, &koff, &klen, &ks);
    const uint32_t NV = (uint32_t)b.vals.size();
    std::vector<uint32_t> ptab((size_t)std::max<uint32_t>(img.memo_words, 1) * (NV + KV_PTAB_PSEUDO), 0u);
    DevPS P{};
    P.prog = ps.prog.data();
    P.preds = ps.preds.data();
    P.alts = ps.alts.data();
    P.conjs = ps.conjs.data();
    P.atoms = ps.atoms.data();
    P.rules = ps.rules.data();
    P.filters = ps.filters.data();
    P.fflags = fflags.data();
    P.kinds = ps.kinds.data();
    P.strrefs = ps.strrefs.data();
    P.strpairs = ps.strpairs.data();
    P.sels = ps.selectors.data();
    P.sellabels = ps.sellabels.data();
    P.selexprs = ps.selexprs.data();
    P.kg_specs = ps.kg_specs.data();
    P.gsegs = ps.gsegs.data();
    P.gwords = ps.gwords.data();
    P.pstr = (const uint8_t*)ps.strs.data();
    P.star_id = ps.lookup("*");
    if (P.star_id == KEY_NONE) P.star_id = KEY_NONE - 1;
    P.n_rules = (uint32_t)ps.rules.size();
    P.n_filters = (uint32_t)ps.filters.size();
    P.n_sels = (uint32_t)ps.selectors.size();
    P.ptab = ptab.data();
    P.n_vals = NV + KV_PTAB_PSEUDO;
    DevBatch B{};
    // the packed rows (what kv_validate uploads), expanded as kv_expand_rows_kernel does
    if (b.rmask.size() != b.n_rows || b.rwide.size() != b.n_rows || b.roff.size() != b.n_rows)
      throw std::runtime_error("kvemu: packed row arrays do not match the batch");
    std::vector<Node> expanded(b.n_cells(), Node{0u, 0u, 0u, 0u});
    for (uint64_t row = 0; row < b.n_rows; row++)
      for (uint32_t l = 0; l < KV_LANES; l++)
        if ((b.rmask[row] >> l) & 1ull) {
          if ((size_t)(b.unit(row, l) - b.tcells.data()) + ((b.rwide[row] >> l) & 1ull) >= b.tcells.size())
            throw std::runtime_error("kvemu: packed cell index out of range");
          expanded[row * KV_LANES + l] = b.cell(row * KV_LANES + l);
        }
    B.nodes = expanded.data();
    B.vals = b.vals.data();
    B.res = b.res.data();
    B.kvs = b.kvs.data();
    B.bstr = (const uint8_t*)b.strs.data();
    B.ns_bits = b.ns_bits.data();
    B.key_off = koff.data();
    B.key_len = klen.data();
    B.kstr = (const uint8_t*)ks.data();
    B.nsms = b.nsms.data();
    B.lsets = b.lsets.data();
    B.asets = b.asets.data();
    B.n_nsm = (uint32_t)b.nsms.size();
    B.n_lsets = (uint32_t)b.lsets.size();
    B.n_asets = (uint32_t)b.asets.size();
    B.ns_words = b.ns_words;
    B.n_res = (uint32_t)b.res.size();
    B.tup_rep = b.tup_rep.data();
    B.n_tup = (uint32_t)b.tup_rep.size();
    B.tup_kent = b.tup_kent.data();
    B.kent_rep = b.kent_rep.data();
    B.n_kent = (uint32_t)b.kent_rep.size();
    B.n_ns = (uint32_t)b.namespaces.size();
    // factored match (as kv_session: descriptors of the image, [slot][entity] tables per type)
    P.fac_word = img.fac_word.data();
    P.fac_bit = img.fac_bit.data();
    P.fac_flist = img.fac_flist.data();
    P.fac_rule = img.fac_rule.data();
    P.fac_slots = img.fac_slots;
    P.fac_words = img.mtup_words;
    std::vector<uint32_t> ftab;
    {
      const uint32_t ne[KV_FAC_TYPES] = {B.n_kent, B.n_nsm, B.n_asets, B.n_lsets, B.n_ns};
      uint64_t at = 0;
      for (uint32_t t = 0; t < KV_FAC_TYPES; t++) {
        P.fac_off[t] = at;
        at += (uint64_t)img.fac_slots * ne[t];
      }
      ftab.assign(std::max<uint64_t>(at, 1), 0xA5A5A5A5u);
      P.fac_tab = ftab.data();
    }
    std::vector<uint32_t> mtup(std::max<size_t>((size_t)img.mtup_words * b.tup_rep.size(), 1), 0xA5A5A5A5u);
    P.mtup = mtup.data();
    P.mtup_words = img.mtup_words;
    // pattern variables (as dev_batch in kvapi.cpp)
    DynHost dyn;
    build_dyn(ps, b, &dyn);
    DevPS PD{};
    PD.preds = dyn.tbl.preds.data();
    PD.alts = dyn.tbl.alts.data();
    PD.conjs = dyn.tbl.conjs.data();
    PD.atoms = dyn.tbl.atoms.data();
    PD.gsegs = dyn.tbl.gsegs.data();
    PD.gwords = dyn.tbl.gwords.data();
    PD.pstr = (const uint8_t*)dyn.tbl.strs.data();
    B.dps = &PD;
    B.dleaf = dyn.dleaf.data();
    B.dyn_st = dyn.dyn_st.data();
    // condition blocks (as dev_batch): the tables, then every (set, resource) through the host
    // twins of kv_precond_kernel, kv_deny_kernel and the foreach kernels (kvcond.h: the per-lane
    // functions the kernels run); the deny plane has the deny sets' rows, then the foreach sets',
    // then the chains' (rules of several entries)
    CondHost pre, dn;
    FeHost fe;
    std::vector<uint8_t> pre_st, deny_st;
    const size_t n_pre = ps.csets.size(), n_dn = ps.dsets.size(), n_fe = ps.fsets.size(), n_ch = ps.fe_chains.size();
    if (n_pre && !b.res.empty()) {
      build_pre(ps, b, &pre);
      pre_st.assign(n_pre * B.n_res, 0xEE);
      for (size_t s = 0; s < n_pre; s++)
        for (uint32_t r = 0; r < B.n_res; r++) pre_st[s * B.n_res + r] = pre_status_host(pre, (uint32_t)s, B.n_res, r);
      B.pre_st = pre_st.data();
    }
    if ((n_dn || n_fe) && !b.res.empty()) {
      build_deny(ps, b, &dn);
      build_foreach(ps, b, &fe);
      deny_st.assign((n_dn + n_fe + n_ch) * B.n_res, 0xEE);
      for (size_t s = 0; s < n_dn; s++)
        for (uint32_t r = 0; r < B.n_res; r++) deny_st[s * B.n_res + r] = deny_status_host(dn, (uint32_t)s, B.n_res, r);
      for (size_t s = 0; s < n_fe; s++)
        for (uint32_t r = 0; r < B.n_res && !ps.fsets[s].pattern && !ps.fsets[s].any; r++)
          deny_st[(n_dn + s) * B.n_res + r] = foreach_fold_host(fe, (uint32_t)s, B.n_res, r, nullptr);
      // (KV_COMPILE_FOREACH_PATVARS, flag 64: the sets with variable strings stand behind the others)
      const FeVarTables vt = fe.var_view(dyn.ityp.data());
      if (!ps.fpats.empty()) {  // (as launch_foreach: the pattern sets' elements through the pattern walk)
        const FeTables ft = fe.view();
        const FePatTables qt = fe.pat_view();
        kvemu_foreach_pat(&ft, &qt, &P, &B, B.n_res, deny_st.data() + n_dn * B.n_res, &vt, ps.n_vpats);
      }
      if (!ps.fanys.empty()) {  // (as launch_foreach: the any sets' elements through their alternatives)
        const FeTables ft = fe.view();
        const FeAnyTables at = fe.any_view();
        kvemu_foreach_any(&ft, &at, &P, &B, B.n_res, deny_st.data() + n_dn * B.n_res, &vt, ps.n_vanys,
                          (uint32_t)ps.fpats.size());
      }
      if (n_ch) {  // (as kv_foreach_chain_kernel, after the set rows: a key per status byte, the element left out)
        std::vector<uint32_t> acc(n_fe * B.n_res);
        for (size_t i = 0; i < acc.size(); i++) {
          const uint8_t st = deny_st[n_dn * B.n_res + i];
          acc[i] = st == ST_PASS ? FE_KEY_PASS : st == ST_SKIP ? FE_KEY_NONE : st;
        }
        const FeTables ft = fe.view();
        for (size_t c = 0; c < n_ch; c++)
          for (uint32_t r = 0; r < B.n_res; r++) {
            uint32_t key;
            deny_st[(n_dn + n_fe + c) * B.n_res + r] = (uint8_t)kv_fe_chain(ft, (uint32_t)c, B.n_res, r, acc.data(), &key);
          }
      }
      B.deny_st = deny_st.data();
    }
    // path columns of the image (as dev_batch: built once per batch)
    std::vector<uint32_t> pcol_erow;
    std::vector<uint32_t> pcol;  // rows by cell format (kvcol.h col_put)
    if (!img.cols.empty() && B.n_res) {
      if (NV + KV_PTAB_PSEUDO >= (1ull << KV_COL_PAYLOAD)) throw std::runtime_error("kvemu: more than 2^28 distinct values");
      pcol = kvemu_pcol(&B, img.cols, img.fam_arr, img.fam_parent, img.fam_ncols, img.fam_nw, img.fam_nb, img.fam_nn, &pcol_erow);
      B.pcol = pcol.data();
    }
    // match tables (as kv_session: one allocation, three [word][entity] tables)
    P.mt_ns_words = (ps.n_nss_bits + 31) / 32;
    P.mt_ann_words = (ps.n_ann_bits + 31) / 32;
    P.mt_sel_words = (uint32_t)((ps.selectors.size() + 31) / 32);
    const size_t n_ns = (size_t)P.mt_ns_words * B.n_nsm, n_an = (size_t)P.mt_ann_words * B.n_asets,
                 n_sl = (size_t)P.mt_sel_words * B.n_lsets;
    std::vector<uint32_t> mt(std::max<size_t>(n_ns + n_an + n_sl, 1), 0xA5A5A5A5u);
    P.mt_ns = mt.data();
    P.mt_ann = mt.data() + n_ns;
    const std::vector<uint32_t> bitf = mtab_bit_filters(ps);
    P.mt_bitf = bitf.data();
    P.mt_sel = mt.data() + n_ns + n_an;
    kvemu_mtab(&P, &B, P.mt_ns_words + P.mt_ann_words + P.mt_sel_words,
               std::max({B.n_nsm, B.n_asets, B.n_lsets}), mt.data(), mt.data() + n_ns, mt.data() + n_ns + n_an);
    const uint64_t nr = ps.rules.size(), nres = b.res.size();

    if (img.memo_words) {
      auto f = (ptab_fn)dlsym(RTLD_DEFAULT, "kvj_ptab");
      if (!f) throw std::runtime_error("kvj_ptab not linked in");
      const uint32_t rows = (uint32_t)((img.memo_preds.size() + img.ptab_row - 1) / img.ptab_row);
      grid((NV + KV_PTAB_PSEUDO + KV_WG - 1) / KV_WG, rows, [&]() { f(&P, B.vals, B.bstr, NV, ptab.data()); });
    }
    if (img.mtup_words && B.n_tup) kvemu_mfac(&P, &B, mtup.data());  // (as kv_session, after the match tables)
    std::vector<uint8_t> status(nr * nres, 0xEE);
    std::vector<ErrRec8> err8(nr * nres);
    std::vector<ErrRec> errw;
    std::vector<unsigned long long> counts(std::max<uint64_t>(nr, 1) * KV_HIST, 0);
    DevOut O{};
    O.status = status.data();
    O.err8 = err8.data();
    O.counts = counts.data();
    O.full = 3;
    std::vector<chunk_fn> fns;
    for (const JitChunk& c : img.chunks) {
      auto f = (chunk_fn)dlsym(RTLD_DEFAULT, c.name.c_str());
      if (!f) throw std::runtime_error(c.name + " not linked in");
      fns.push_back(f);
    }
    const uint32_t blocks = (uint32_t)((nres + KV_RWG - 1) / KV_RWG);
    auto pass = [&]() {
      for (chunk_fn f : fns) grid(blocks, 1, [&]() { f(&P, &B, B.nodes, B.vals, B.bstr, O, 0u); }, (uint32_t)KV_RWG);
    };
    if (nres) pass();
    bool wide = false;
    for (size_t o = 0; o < status.size() && !wide; o++) {
      const uint8_t s = status[o];
      wide = (s == ST_FAIL || s == ST_ERROR || s == ST_SKIP) && (err8[o].w0 & ERR8_WIDE);
    }
    // KVEMU_NO_ERR=1: statuses only (large batches); the wide re-pass still runs
    const bool want_err = !getenv("KVEMU_NO_ERR");
    if (want_err || wide) errw.assign(nr * nres, ErrRec{});
    if (wide) {  // as kv_session::fetch: one more pass writing full records
      O.err = errw.data();
      O.full |= 4;
      pass();
    }
    for (size_t o = 0; o < status.size() && want_err; o++) {
      const uint8_t s = status[o];
      if (!(s == ST_FAIL || s == ST_ERROR || s == ST_SKIP) || (err8[o].w0 & ERR8_WIDE)) continue;
      const ErrRec8 c = err8[o];
      ErrRec e{};
      e.kind_flags = (c.w0 & 15u) | (((c.w0 >> 4) & 3u) << 16);
      e.pnode = c.w0 >> 7;
      e.keynode = ABSENT;
      e.resnode = ABSENT;
      e.idx[0] = c.w1 & 1023u;
      e.idx[1] = (c.w1 >> 10) & 255u;
      e.idx[2] = (c.w1 >> 18) & 255u;
      errw[o] = e;
    }
    wide_any |= wide;
    for (uint64_t rl = 0; rl < nr; rl++) {
      memcpy(status_all.data() + rl * n_total + lo, status.data() + rl * nres, nres);
      if (want_err_all)
        for (uint64_t q = 0; q < nres; q++) err_all[rl * n_total + lo + q] = errw[rl * nres + q];
    }
    }  // shards
    const uint64_t nr = ps.rules.size(), nres = n_total;
    const bool wide = wide_any;
    if (!order.empty()) {  // store order -> the input's resource order (as kv_result_status)
      std::vector<uint8_t> st(status_all.size());
      std::vector<ErrRec> ew(err_all.size());
      for (uint64_t rl = 0; rl < nr; rl++)
        for (uint64_t q = 0; q < nres; q++) {
          st[rl * nres + order[q]] = status_all[rl * nres + q];
          if (!err_all.empty()) ew[rl * nres + order[q]] = err_all[rl * nres + q];
        }
      status_all.swap(st);
      err_all.swap(ew);
    }
    const std::vector<uint8_t>& status = status_all;
    const std::vector<ErrRec>& errw = err_all;
    const std::string out = argv[4];
    FILE* fs = fopen((out + ".status").c_str(), "wb");
    FILE* fe = fopen((out + ".err").c_str(), "wb");
    FILE* fm = fopen((out + ".meta").c_str(), "w");
    if (!fs || !fe || !fm) throw std::runtime_error("cannot write outputs");
    fwrite(status.data(), 1, status.size(), fs);
    fwrite(errw.data(), sizeof(ErrRec), errw.size(), fe);
    fprintf(fm, "%llu %llu %d\n", (unsigned long long)nr, (unsigned long long)nres, wide ? 1 : 0);
    fclose(fs);
    fclose(fe);
    fclose(fm);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "kvemu: %s\n", e.what());
    return 1;
  }
}
