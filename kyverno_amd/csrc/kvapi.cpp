// C ABI (include/kvgpu.h) + device runtime: HBM residency of compiled policy
// sets and ingested batches, launch-time folding of batch-constant user info,
// sessions. (Pools: kvmem.cpp; host-side reading of a fetched result: kvresult.cpp.)
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <cstdio>
#include <cstring>

#define KVRT_DEVICE 1
#include "kvrt.hpp"
#include "kvdev.h"

namespace kvh {

struct DevPolicySet {
  DevBuf prog, preds, alts, conjs, atoms, rules, filters, kinds, strrefs, strpairs, sels, sellabels, selexprs, kgs,
      gsegs, gwords, pstr, fword, fbit, flist, frule, rcompact, gsdesc, gsmem;
  DevBuf view_dev;  // `view` on the device (without the per-session tables): what kv_foreach_pat_kernel walks
  // site-record groups of the specialized kernels (kvdevtypes.h GSiteDesc)
  uint32_t gs_groups = 0, gs_members = 0;
  DevPS view{};
  // specialized kernels (KV_COMPILE_SPECIALIZE): one module per kernel program, one
  // function per rule chunk
  std::vector<hipModule_t> mods;
  std::vector<hipFunction_t> fns;
  // output-mode variants (JitImage::variants): DevOut::full value -> a function per rule kernel
  // (the variant where it compiled within the plan's registers, else the generic kernel)
  std::map<uint32_t, std::vector<hipFunction_t>> vfns;
  const std::vector<hipFunction_t>& fns_for(uint32_t full) const {
    auto it = vfns.find(full);
    return it == vfns.end() ? fns : it->second;
  }
  // the rule kernels longest first, as the first session to time them found (DevSession::
  // order_kernels); later sessions of the policy set on this device, kv_validate's single pass
  // included, start from it
  std::mutex order_mu;
  std::vector<uint32_t> korder;
  hipFunction_t ptab_fn = nullptr;  // value-predicate table builder (kvj_ptab)
  uint32_t mtup_words = 0;          // match words per tuple (kv_mfac + kv_mtup, factored match)
  uint32_t fac_slots = 0;
  uint32_t memo_words = 0, ptab_rows = 0;
  int dev = -1;
  bool specialized() const { return !mods.empty(); }
  ~DevPolicySet() {
    if (!mods.empty()) {
      int cur;
      if (hipGetDevice(&cur) == hipSuccess) {
        (void)hipSetDevice(dev);
        for (hipModule_t m : mods) (void)hipModuleUnload(m);
        (void)hipSetDevice(cur);
      }
    }
  }
};

struct DevBatchRes {
  DevBuf nodes, vals, res, kvs, bstr, nsbits, koff, klen, kstr, nsms, lsets, asets, tuprep, tupkent, kentrep, view_dev;
  // pattern variables (kvvars.cpp): the batch predicate table (a DevPS with its pred tables),
  // outcome ids per [dynamic leaf][res], statuses per [dynamic rule][res]
  DevBuf dpreds, dalts, dconjs, datoms, dgsegs, dgwords, dpstr, dps, dleaf, dynst;
  // path columns of the specialized kernels (kvcol.h): the pool, the column descriptors, the
  // families and their per-group element-row prefixes; build time and pool size
  DevBuf pcol, pcold, pfam, perow;
  double pcol_ms = 0;
  // condition blocks (kvcond.h): the tables of the gate, of validate.deny and of validate.foreach
  // (its gate and deny blocks, its own five tables, the reduction keys fe_acc[set][res]), each
  // list in its host struct's order; the plane kv_precond_kernel wrote, and the one kv_deny_kernel
  // (rows of the deny sets) and the foreach kernels (rows after them) wrote; HIP-event times
  // pattern sets (KV_COMPILE_FOREACH_PATTERN): their three tables and fe_rec[pattern set][res]
  DevBuf pre[5], dn[7], feg[2], fed[7], fe[5], fep[3], feacc, ferec, prest, dnst;
  // rules of several entries (KV_COMPILE_FOREACH_ENTRIES): the chain tables and fe_ckey[chain][res]
  DevBuf fec[2], feckey;
  // any sets (KV_COMPILE_FOREACH_ANYPATTERN): their two tables (the list paths and `first` are the
  // pattern sets' buffers), fe_acode[any set][res] and fe_arec[alternative][res]
  DevBuf fea[2], feacode, fearec;
  // variable strings in entries' patterns (KV_COMPILE_FOREACH_PATVARS): the runs, their rows, the M
  // plane and the int-typing plane of the batch predicate table
  DevBuf fev[4];
  double pre_ms = 0, deny_ms = 0, fe_ms = 0;
  DevBatch view{};
};
}  // namespace kvh

kv_policyset::kv_policyset() = default;
kv_policyset::~kv_policyset() = default;

namespace {

DevPolicySet& dev_ps(kv_policyset* s, int device) {
  std::lock_guard<std::mutex> g(s->mu);
  auto it = s->dev.find(device);
  if (it != s->dev.end()) return *it->second;
  auto d = std::make_unique<DevPolicySet>();
  const PolicySet& ps = s->ps;
  d->prog.upload(ps.prog, device);
  d->preds.upload(ps.preds, device);
  d->alts.upload(ps.alts, device);
  d->conjs.upload(ps.conjs, device);
  d->atoms.upload(ps.atoms, device);
  d->rules.upload(ps.rules, device);
  d->filters.upload(ps.filters, device);
  d->kinds.upload(ps.kinds, device);
  d->strrefs.upload(ps.strrefs, device);
  d->strpairs.upload(ps.strpairs, device);
  d->sels.upload(ps.selectors, device);
  d->sellabels.upload(ps.sellabels, device);
  d->selexprs.upload(ps.selexprs, device);
  d->kgs.upload(ps.kg_specs, device);
  d->gsegs.upload(ps.gsegs, device);
  d->gwords.upload(ps.gwords, device);
  d->pstr.upload_raw(ps.strs.data(), ps.strs.size(), device);
  DevPS& v = d->view;
  v.prog = (const Inst*)d->prog.p;
  v.preds = (const Pred*)d->preds.p;
  v.alts = (const Alt*)d->alts.p;
  v.conjs = (const Conj*)d->conjs.p;
  v.atoms = (const Atom*)d->atoms.p;
  v.rules = (const RuleRec*)d->rules.p;
  v.filters = (const MFilter*)d->filters.p;
  v.kinds = (const KindSpec*)d->kinds.p;
  v.strrefs = (const StrRef*)d->strrefs.p;
  v.strpairs = (const StrPair*)d->strpairs.p;
  v.sels = (const Selector*)d->sels.p;
  v.sellabels = (const SelLabel*)d->sellabels.p;
  v.selexprs = (const SelExpr*)d->selexprs.p;
  v.kg_specs = (const uint32_t*)d->kgs.p;
  v.gsegs = (const GSeg*)d->gsegs.p;
  v.gwords = (const GWord*)d->gwords.p;
  v.n_rules = (uint32_t)ps.rules.size();
  v.n_filters = (uint32_t)ps.filters.size();
  v.n_sels = (uint32_t)ps.selectors.size();
  v.pstr = (const uint8_t*)d->pstr.p;
  // resource version "*" (checkKind, pkg/engine/utils.go:49): when "*" is not in the key dictionary no
  // resource can carry it, and an unknown version (KEY_NONE) must not compare equal to it
  v.star_id = ps.lookup("*");
  if (v.star_id == KEY_NONE) v.star_id = KEY_NONE - 1;
  d->dev = device;
  if (s->jit) {
    const JitImage& J = *s->jit;
    std::map<std::string, hipFunction_t> byname;
    for (size_t i = 0; i < J.codes.size(); i++) {
      hipModule_t m;
      HIPCHK(hipModuleLoadData(&m, J.codes[i].data()));
      d->mods.push_back(m);
      hipFunction_t f;
      HIPCHK(hipModuleGetFunction(&f, m, J.kernel_name[i].c_str()));
      byname[J.kernel_name[i]] = f;
    }
    for (const JitImage::Variant& v : J.variants) {
      std::map<std::string, hipFunction_t> vname;
      for (size_t i = 0; i < v.codes.size() && i < J.kernel_name.size(); i++) {
        if (v.codes[i].empty()) continue;
        hipModule_t m;
        HIPCHK(hipModuleLoadData(&m, v.codes[i].data()));
        d->mods.push_back(m);
        hipFunction_t f;
        HIPCHK(hipModuleGetFunction(&f, m, J.kernel_name[i].c_str()));
        vname[J.kernel_name[i]] = f;
      }
      std::vector<hipFunction_t>& fv = d->vfns[v.full];
      for (auto& ch : J.chunks) {
        auto it = vname.find(ch.name);
        fv.push_back(it != vname.end() ? it->second : byname.at(ch.name));
      }
    }
    for (auto& ch : J.chunks) {
      auto it = byname.find(ch.name);
      if (it == byname.end()) throw std::runtime_error("specialized kernel " + ch.name + " missing");
      hipFunction_t f = it->second;
      d->fns.push_back(f);
      if (getenv("KVGPU_VERBOSE")) {  // register / scratch use of each specialized kernel
        int regs = 0, local = 0;
        (void)hipFuncGetAttribute(&regs, HIP_FUNC_ATTRIBUTE_NUM_REGS, f);
        (void)hipFuncGetAttribute(&local, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, f);
        fprintf(stderr, "[kvgpu] %s: %zu rules, %d VGPRs, %d B scratch/lane\n", ch.name.c_str(), ch.rules.size(), regs,
                local);
      }
    }
    d->rcompact.upload(J.rec_compact, device);  // record layout per rule (JitImage::rec_compact)
    if (!J.gs_desc.empty()) {
      d->gs_groups = (uint32_t)(J.gs_desc.size() / 4u);
      d->gs_members = J.gs_members;
      d->gsdesc.upload(J.gs_desc, device);
      d->gsmem.upload(J.gs_mem, device);
    }
    if (J.mtup_words) {  // factored-match descriptors of the kernels' match bits
      d->mtup_words = J.mtup_words;
      d->fac_slots = J.fac_slots;
      d->fword.upload(J.fac_word, device);
      d->fbit.upload(J.fac_bit, device);
      d->flist.upload(J.fac_flist, device);
      d->frule.upload(J.fac_rule, device);
      v.fac_word = (const uint32_t*)d->fword.p;
      v.fac_bit = (const uint32_t*)d->fbit.p;
      v.fac_flist = (const uint32_t*)d->flist.p;
      v.fac_rule = (const uint32_t*)d->frule.p;
      v.fac_slots = J.fac_slots;
      v.fac_words = J.mtup_words;
    }
    if (J.memo_words) {
      d->ptab_fn = byname.at("kvj_ptab");
      d->memo_words = J.memo_words;
      d->ptab_rows = (uint32_t)((J.memo_preds.size() + J.ptab_row - 1) / J.ptab_row);
    }
  }
  if (!ps.fpats.empty() || !ps.fanys.empty()) d->view_dev.upload_raw(&d->view, sizeof(DevPS), device);
  auto& ref = *d;
  s->dev[device] = std::move(d);
  return ref;
}

// Path columns of the batch for the policy set's specialized kernels (kvcol.h, kvdevtypes.h):
// the rows of family 0, one per wave group (wave groups padded to whole workgroups, so every lane
// of the rule kernels' grid has its cells), then each family's element rows (a nested family's:
// one run of rows per row of its parent); built once per batch and device from the node rows
// (d->view_dev must hold the batch view).
void build_pcol(const JitImage& J, const Batch& b, DevBatchRes* d, int device) {
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t nf = (uint32_t)J.fam_ncols.size(), j0 = J.fam_ncols.at(0);
  const uint64_t groups64 = (b.res.size() + KV_WG - 1) / KV_WG * (KV_WG / KV_LANES);
  if (groups64 > 0x3FFFFFFull) throw std::runtime_error("path columns: too many resources");
  const uint32_t groups = (uint32_t)groups64;
  d->pcold.upload(J.cols, device);
  d->perow.alloc((size_t)std::max<uint32_t>(1u, nf - 1) * (groups + 1) * sizeof(uint32_t), device);
  HIPCHK(hipMemset(d->perow.p, 0, d->perow.n));
  std::vector<ColFam> fams(nf);
  uint32_t n_wide = 0, n_narrow = 0;
  bool nested = false;
  for (uint32_t f = 0; f < nf; f++) {
    fams[f].arr_col = J.fam_arr[f];
    fams[f].parent = J.fam_parent.at(f);
    nested = nested || fams[f].parent != 0;
    fams[f].ncols = J.fam_ncols[f];
    fams[f].nw = J.fam_nw.at(f);
    fams[f].nb = J.fam_nb.at(f);
    fams[f].nn = J.fam_nn.at(f);
    fams[f].erow = f ? (uint32_t*)d->perow.p + (size_t)(f - 1) * (groups + 1) : nullptr;
    n_wide += fams[f].nw;
    n_narrow += fams[f].nn;
  }
  // (a narrow cell holds a Val id in KV_COL_PAYLOAD bits)
  if (n_narrow && b.vals.size() + KV_PTAB_PSEUDO >= (1ull << KV_COL_PAYLOAD))
    throw std::runtime_error("path columns: more than 2^28 distinct values");
  d->pfam.upload(fams, device);
  const DevBatch* Bd = (const DevBatch*)d->view_dev.p;
  const ColDesc* cd = (const ColDesc*)d->pcold.p;
  std::vector<uint32_t> erow;
  if (nf > 1) {
    // (the rows of every family, nested ones included, come back in this one copy)
    HIPCHK(launch_pcol_rows(Bd, cd, (const ColFam*)d->pfam.p, nf, nested, groups, nullptr));
    erow.resize((size_t)(nf - 1) * (groups + 1));
    HIPCHK(hipMemcpy(erow.data(), d->perow.p, erow.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  auto row_words = [&](uint32_t f) { return (uint64_t)(3u * fams[f].nw + fams[f].nb + fams[f].nn) * KV_LANES; };
  const uint64_t root_words = (uint64_t)groups * row_words(0);
  uint64_t words = root_words;
  for (uint32_t f = 1; f < nf; f++) {
    fams[f].off_lo = (uint32_t)words;
    fams[f].off_hi = (uint32_t)(words >> 32);
    words += (uint64_t)erow[(size_t)(f - 1) * (groups + 1) + groups] * row_words(f);
  }
  // (the kernels index the pool's words with 32 bits)
  if (words >= (1ull << 32)) throw std::runtime_error("path columns: more than 2^32 words");
  HIPCHK(hipMemcpy(d->pfam.p, fams.data(), fams.size() * sizeof(ColFam), hipMemcpyHostToDevice));
  d->pcol.alloc(std::max<uint64_t>(words, 1) * sizeof(uint32_t), device);
  uint32_t* pool = (uint32_t*)d->pcol.p;
  // element rows past a lane's own elements stay zero
  if (words > root_words) HIPCHK(hipMemset(pool + root_words, 0, (words - root_words) * sizeof(uint32_t)));
  HIPCHK(launch_pcol_build(Bd, cd, (const ColFam*)d->pfam.p, 0, j0, groups, 0u, pool, nullptr));
  for (uint32_t level = 1; level <= (nested ? 2u : 1u); level++)
    HIPCHK(launch_pcol_build(Bd, cd, (const ColFam*)d->pfam.p, j0, (uint32_t)J.cols.size() - j0, groups, level, pool,
                             nullptr));
  HIPCHK(hipStreamSynchronize(nullptr));
  d->view.pcol = pool;
  d->pcol_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (getenv("KVGPU_VERBOSE"))
    fprintf(stderr,
            "[kvgpu] path columns: %u wide + %u narrow columns in %u families, %llu bytes (%.1f per resource), built in "
            "%.2f ms\n",
            n_wide, n_narrow, nf, (unsigned long long)(words * sizeof(uint32_t)),
            b.res.empty() ? 0.0 : (double)(words * sizeof(uint32_t)) / (double)b.res.size(), d->pcol_ms);
}

// pdev: the policy set's device view (DevPolicySet::view_dev), read by the pattern sets' kernel
std::shared_ptr<DevBatchRes> dev_batch(kv_batch* bt, const PolicySet& ps, int device, const DevPS* pdev) {
  std::lock_guard<std::mutex> g(bt->mu);
  auto it = bt->dev.find(device);
  if (it != bt->dev.end()) return it->second;
  auto d = std::make_shared<DevBatchRes>();
  const Batch& b = bt->b;
  if (b.rmask.size() != b.n_rows || b.rwide.size() != b.n_rows || b.roff.size() != b.n_rows)
    throw std::runtime_error("batch: packed row arrays do not match the row count");
  // packed rows: upload the non-zero cells, masks and row offsets, then expand to the
  // wave-group layout on the device. The page-locked arrays (rows, values, resources) go as
  // asynchronous copies on one stream, the expansion behind them, while this thread uploads the
  // pageable ones (strings, key table, match inputs) through the staging path beside them.
  hipStream_t us = StreamPool::get().take(device, hipStreamNonBlocking);
  DevBuf pc, rm, rw, ro;
  pc.upload_async(b.tcells, device, us);
  rm.upload_async(b.rmask, device, us);
  rw.upload_async(b.rwide, device, us);
  ro.upload_async(b.roff, device, us);
  d->vals.upload_async(b.vals, device, us);
  d->nodes.alloc(b.n_cells() * sizeof(Node), device);
  HIPCHK(launch_expand_rows((const uint64_t*)pc.p, (const uint64_t*)rm.p, (const uint64_t*)rw.p, (const uint32_t*)ro.p,
                            (const Val*)d->vals.p, b.n_rows, (Node*)d->nodes.p, us));
  d->res.upload_async(b.res, device, us);
  d->kvs.upload(b.kvs, device);
  d->bstr.upload_raw(b.strs.data(), b.strs.size(), device);
  d->nsbits.upload(b.ns_bits, device);
  // key string table: static dictionary then batch-dynamic keys
  std::vector<uint32_t> off, len;
  std::string ks;
  key_table(ps, b, &off, &len, &ks);
  d->koff.upload(off, device);
  d->klen.upload(len, device);
  d->kstr.upload_raw(ks.data(), ks.size(), device);
  d->nsms.upload(b.nsms, device);
  d->lsets.upload(b.lsets, device);
  d->asets.upload(b.asets, device);
  d->tuprep.upload(b.tup_rep, device);
  d->tupkent.upload(b.tup_kent, device);
  d->kentrep.upload(b.kent_rep, device);
  DevBatch& v = d->view;
  v.nodes = (const Node*)d->nodes.p;
  v.vals = (const Val*)d->vals.p;
  v.res = (const Res*)d->res.p;
  v.kvs = (const KV*)d->kvs.p;
  v.bstr = (const uint8_t*)d->bstr.p;
  v.ns_bits = (const uint32_t*)d->nsbits.p;
  v.key_off = (const uint32_t*)d->koff.p;
  v.key_len = (const uint32_t*)d->klen.p;
  v.kstr = (const uint8_t*)d->kstr.p;
  v.nsms = (const StrRef*)d->nsms.p;
  v.lsets = (const KVSet*)d->lsets.p;
  v.asets = (const KVSet*)d->asets.p;
  v.n_nsm = (uint32_t)b.nsms.size();
  v.n_lsets = (uint32_t)b.lsets.size();
  v.n_asets = (uint32_t)b.asets.size();
  v.ns_words = b.ns_words;
  v.n_res = (uint32_t)b.res.size();
  v.tup_rep = (const uint32_t*)d->tuprep.p;
  v.n_tup = (uint32_t)b.tup_rep.size();
  v.tup_kent = (const uint32_t*)d->tupkent.p;
  v.kent_rep = (const uint32_t*)d->kentrep.p;
  v.n_kent = (uint32_t)b.kent_rep.size();
  v.n_ns = (uint32_t)b.namespaces.size();
  {  // pattern variables: every pointer valid (16-byte buffers when the policy set has none)
    const DynHost& h = bt->dyn_host(ps);
    d->dpreds.upload(h.tbl.preds, device);
    d->dalts.upload(h.tbl.alts, device);
    d->dconjs.upload(h.tbl.conjs, device);
    d->datoms.upload(h.tbl.atoms, device);
    d->dgsegs.upload(h.tbl.gsegs, device);
    d->dgwords.upload(h.tbl.gwords, device);
    d->dpstr.upload_raw(h.tbl.strs.data(), h.tbl.strs.size(), device);
    DevPS dv{};
    dv.preds = (const Pred*)d->dpreds.p;
    dv.alts = (const Alt*)d->dalts.p;
    dv.conjs = (const Conj*)d->dconjs.p;
    dv.atoms = (const Atom*)d->datoms.p;
    dv.gsegs = (const GSeg*)d->dgsegs.p;
    dv.gwords = (const GWord*)d->dgwords.p;
    dv.pstr = (const uint8_t*)d->dpstr.p;
    d->dps.upload_raw(&dv, sizeof(DevPS), device);
    d->dleaf.upload(h.dleaf, device);
    d->dynst.upload(h.dyn_st, device);
    v.dps = (const DevPS*)d->dps.p;
    v.dleaf = (const uint32_t*)d->dleaf.p;
    v.dyn_st = (const uint8_t*)d->dynst.p;
  }
  // condition blocks: their tables go on the upload stream (no blocking copy; the host structs live
  // until the stream is drained below), the kernels behind them. The deny plane has a row per deny
  // set, then per foreach set.
  auto up = [&](DevBuf* bufs, std::initializer_list<const std::vector<uint32_t>*> src, const uint32_t** dp) {
    for (const std::vector<uint32_t>* v : src) {
      bufs->alloc(std::max<size_t>(v->size() * sizeof(uint32_t), 16), device);
      if (!v->empty()) HIPCHK(hipMemcpyAsync(bufs->p, v->data(), v->size() * sizeof(uint32_t), hipMemcpyHostToDevice, us));
      *dp++ = (const uint32_t*)(bufs++)->p;
    }
  };
  auto up_blocks = [&](DevBuf* bufs, const CondHost& h, bool strict) {  // (a gate has no err / oos planes)
    const uint32_t* dp[7] = {};
    up(bufs, {&h.sets, &h.ents, &h.outc, &h.truth, &h.unk}, dp);
    if (strict) up(bufs + 5, {&h.err, &h.oos}, dp + 5);
    return CondBlocks{dp[0], dp[1], dp[2], dp[3], dp[4], dp[5], dp[6], h.words};
  };
  struct Timed {
    hipEvent_t e0, e1;
    double* ms;
  };
  std::vector<Timed> timed;
  auto timed_launch = [&](double* ms, auto&& launch) {
    Timed t{nullptr, nullptr, ms};
    HIPCHK(hipEventCreate(&t.e0));
    HIPCHK(hipEventCreate(&t.e1));
    HIPCHK(hipEventRecord(t.e0, us));
    HIPCHK(launch());
    HIPCHK(hipEventRecord(t.e1, us));
    timed.push_back(t);
  };
  CondHost pre, dn;
  FeHost fh;
  CondBlocks pt{}, dt{};
  FeTables ft{};
  FePatTables qt{};
  DevBuf erec;  // the pattern sets' per-element records: needed until the fold's kernels are done
  FeAnyTables at{};
  DevBuf acode, arec;  // the any sets' per-element code words and records: likewise
  FeVarTables vt{};
  const uint32_t n_sets = (uint32_t)ps.csets.size(), n_dsets = (uint32_t)ps.dsets.size(),
                 n_fsets = (uint32_t)ps.fsets.size(), n_pats = (uint32_t)ps.fpats.size(),
                 n_anys = (uint32_t)ps.fanys.size(),
                 n_chains = (uint32_t)ps.fe_chains.size();
  if (n_sets && !b.res.empty()) {
    build_pre(ps, b, &pre);
    pt = up_blocks(d->pre, pre, false);
    d->prest.alloc((size_t)n_sets * b.res.size(), device);
    v.pre_st = (const uint8_t*)d->prest.p;
  }
  if (n_dsets && !b.res.empty()) {
    build_deny(ps, b, &dn);
    dt = up_blocks(d->dn, dn, true);
  }
  if (n_fsets && !b.res.empty()) {
    build_foreach(ps, b, &fh);
    // (allocation order matters to what the buffer pool hands the next batch: keep it)
    const uint32_t *dp[5], *gp[2];
    up(d->fe, {&fh.sets, &fh.lists}, dp);
    up(d->feg, {&fh.gate.sets, &fh.gate.ents}, gp);
    ft = fh.view();
    ft.gate = ft.deny = up_blocks(d->fed, fh.deny, true);
    ft.gate.sets = gp[0]; ft.gate.ents = gp[1];
    up(d->fe + 2, {&fh.el_res, &fh.el_ord, &fh.lstate}, dp + 2);
    ft.sets = dp[0]; ft.lists = dp[1]; ft.el_res = dp[2]; ft.el_ord = dp[3]; ft.lstate = dp[4];
    d->feacc.alloc((size_t)n_fsets * b.res.size() * sizeof(uint32_t), device);
    if (n_pats || n_anys) {
      const uint32_t* qp[3];
      up(d->fep, {&fh.pats, &fh.chain, &fh.first}, qp);
      qt = FePatTables{qp[0], qp[1], qp[2], n_pats};
    }
    if (n_pats) {
      erec.alloc(std::max<size_t>((size_t)n_pats * fh.max_el * sizeof(ErrRec8), 16), device);
      d->ferec.alloc((size_t)n_pats * b.res.size() * sizeof(ErrRec8), device);
    }
    if (n_anys) {
      const uint32_t* ap[2];
      up(d->fea, {&fh.anys, &fh.any_alts}, ap);
      const size_t n_alts = fh.any_alts.size();
      at = FeAnyTables{ap[0], ap[1], qt.chain, qt.first, n_anys, (uint32_t)n_alts};
      acode.alloc(std::max<size_t>((size_t)n_anys * fh.max_el * sizeof(uint32_t), 16), device);
      arec.alloc(std::max<size_t>(n_alts * fh.max_el * sizeof(ErrRec8), 16), device);
      d->feacode.alloc((size_t)n_anys * b.res.size() * sizeof(uint32_t), device);
      d->fearec.alloc(n_alts * b.res.size() * sizeof(ErrRec8), device);
    }
    // (one source of truth for the launch split: the policy set's counts; tables that disagree
    // would send sets with variables through the kernels without them)
    if ((ps.n_vpats || ps.n_vanys) != fh.has_vars())
      throw std::runtime_error("foreach tables: variable-string runs do not match the policy set");
    if (ps.n_vpats || ps.n_vanys) {
      const uint32_t* vp[4];
      up(d->fev, {&fh.vruns, &fh.vrows, &fh.mpl, &bt->dyn_host(ps).ityp}, vp);
      vt = FeVarTables{vp[0], vp[1], vp[2], vp[3]};
    }
    if (n_chains) {
      const uint32_t* cp[2];
      up(d->fec, {&fh.chains, &fh.chain_ents}, cp);
      ft.chains = cp[0]; ft.chain_ents = cp[1];
      d->feckey.alloc((size_t)n_chains * b.res.size() * sizeof(uint32_t), device);
    }
  }
  if ((n_dsets || n_fsets) && !b.res.empty()) {
    d->dnst.alloc((size_t)(n_dsets + n_fsets + n_chains) * b.res.size(), device);
    v.deny_st = (const uint8_t*)d->dnst.p;
  }
  d->view_dev.upload_raw(&d->view, sizeof(DevBatch), device);
  if (v.pre_st) timed_launch(&d->pre_ms, [&]() { return launch_cond(false, pt, v.n_res, n_sets, (uint8_t*)d->prest.p, us); });
  if (v.deny_st && n_dsets)
    timed_launch(&d->deny_ms, [&]() { return launch_cond(true, dt, v.n_res, n_dsets, (uint8_t*)d->dnst.p, us); });
  if (v.deny_st && n_fsets)
    timed_launch(&d->fe_ms, [&]() {
      return launch_foreach(ft, v.n_res, (uint32_t*)d->feacc.p, (uint8_t*)d->dnst.p + (size_t)n_dsets * v.n_res, us,
                            n_pats ? &qt : nullptr, pdev, (const DevBatch*)d->view_dev.p, (uint2*)erec.p,
                            (uint2*)d->ferec.p, (uint8_t*)d->dnst.p + (size_t)(n_dsets + n_fsets) * v.n_res,
                            (uint32_t*)d->feckey.p, n_anys ? &at : nullptr, (uint32_t*)acode.p, (uint2*)arec.p,
                            (uint32_t*)d->feacode.p, (uint2*)d->fearec.p, ps.n_vpats || ps.n_vanys ? &vt : nullptr,
                            ps.n_vpats, ps.n_vanys);
    });
  HIPCHK(hipStreamSynchronize(us));
  for (const Timed& t : timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, t.e0, t.e1));
    *t.ms = ms;
    (void)hipEventDestroy(t.e0);
    (void)hipEventDestroy(t.e1);
  }
  StreamPool::get().give(device, hipStreamNonBlocking, us);
  pc.release();
  rm.release();
  rw.release();
  ro.release();
  if (bt->owner && bt->owner->jit && !bt->owner->jit->cols.empty() && !b.res.empty()) {
    build_pcol(*bt->owner->jit, b, d.get(), device);
    d->view_dev.upload_raw(&d->view, sizeof(DevBatch), device);
  }
  bt->dev[device] = d;
  return d;
}

// A launch configuration on one device over one batch (a whole batch or a
// shard): device-resident inputs and output buffers.
struct DevSession {
  kv_policyset* ps = nullptr;
  kv_batch* bt = nullptr;
  int device = 0;
  uint32_t mode = 0;
  uint64_t nrules = 0, nres = 0;
  DevBuf fflags, pview, st, er8, er, cn, scope, scn, ptab, mtab, mtbf, mtup, ftab;
  // The per-pass tables of the specialized kernels (value-predicate table kvj_ptab, match tables
  // kv_mtab / kv_mfac / kv_mtup) are double-buffered between consecutive passes (ptab / ptab1,
  // mtab / mtab1, ... read through pview / pview1): pass i + 1's tables are built on `pside` while
  // pass i's rule kernels run, waiting only for pass i - 1's rule kernels (the last readers of
  // their buffers), so their waves fill the workgroup slots the rule kernels' last round leaves
  // idle. ev_pt[b]: tables b built; ev_rk[b]: the rule kernels that read tables b done.
  // KVGPU_PTAB_PIPE=0: one set, built ahead of each pass's rule kernels (ptab on the session
  // stream, the match tables on `side`).
  DevBuf ptab1, pview1, mtab1, mtup1, ftab1, cn1, scn1;  // (counts of set 1: zeroed with its tables)
  uint32_t *mt1_ns = nullptr, *mt1_ann = nullptr, *mt1_sel = nullptr;
  hipStream_t pside = nullptr;
  hipEvent_t ev_pt[2] = {nullptr, nullptr}, ev_rk[2] = {nullptr, nullptr};
  bool ptab_pipe = false;
  uint32_t fac_entities = 0, ntup = 0;
  bool rec_compact = false;  // the last pass wrote records per wave segment (specialized kernels)
  // the batch's device copy, shared with the batch's cache and other sessions on it; a part of a
  // parts session keeps it after dropping the batch (detach_batch): the caller's host batch may
  // be freed once the part is attached
  std::shared_ptr<DevBatchRes> batch_ref;
  DevBuf r_offs, r_tot, r_base, r_out8, r_outw, r_wide;  // record compaction (fetch)
  DevBuf r_tkey, r_raw, r_nbase, r_code, r_out8b;        // record codes (fetch)
  DevBuf s_ccnt, s_cbase, s_pack;                        // status transfer form (fetch)
  HostArray<uint8_t> hstage;                             // page-locked staging of the fetch's small copies
  DevBuf inv_d, stc;                                     // caller-order statuses (fetch)
  DevBuf ord_d, r_mask;                                  // caller-order records: batch order, record lanes
  DevBuf stamps;                                         // KVGPU_STAMPS diagnostics
  DevBuf gsite, gcnt;                                    // site records of rule groups (pass)
  DevBuf sflag;                                          // written status segments (specialized)
  uint32_t mt_words = 0, mt_entities = 0;
  uint32_t *mt_ns = nullptr, *mt_ann = nullptr, *mt_sel = nullptr;
  uint32_t nscopes = 0, nvals = 0;
  DevOut O{};
  const DevBatch* bview = nullptr;
  const DevBatch* bhost = nullptr;  // host copy of the batch view (device pointers)
  DevPolicySet* dps = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  // specialized passes: the match tables (kv_mtab, kv_mfac, kv_mtup) run on `side` while
  // `stream` builds the value-predicate table (kvj_ptab); the rule kernels wait for both
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_rkf = nullptr, ev_rkj[3] = {};  // rule kernels over several streams (launch_specialized)
  std::vector<hipStream_t> rkx;                  // (the streams beyond `stream` and `side`)
  std::vector<hipEvent_t> kev;                   // start / end of each rule kernel in the timed pass
  std::vector<uint32_t> korder;                  // rule kernels, longest first (after a timed pass)
  bool ktiming = false;

  double upload_ms = 0;  // policy set + batch upload of the constructor (path columns included)
  DevSession(kv_policyset* p, kv_batch* b, const char* ctx_json, int dev, uint32_t m)
      : ps(p), bt(b), device(dev), mode(m) {
    HIPCHK(hipSetDevice(device));
    const auto tc0 = std::chrono::steady_clock::now();
    DevPolicySet& dp = dev_ps(ps, device);
    batch_ref = dev_batch(bt, ps->ps, device, (const DevPS*)dp.view_dev.p);
    DevBatchRes& db = *batch_ref;
    upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc0).count();
    if (getenv("KVGPU_VERBOSE")) fprintf(stderr, "[kvgpu] session: policy set + batch upload %.1f ms\n", upload_ms);
    bview = (const DevBatch*)db.view_dev.p;
    bhost = &db.view;
    dps = &dp;
    fflags.upload(fold_filters(ps->ps, ctx_json), device);
    DevPS P = dp.view;
    P.fflags = (const uint32_t*)fflags.p;
    if (dp.ptab_fn) {  // value-predicate table of the specialized kernels: memo_words per distinct value
      nvals = (uint32_t)bt->b.vals.size();
      ptab.alloc((size_t)dp.memo_words * (nvals + KV_PTAB_PSEUDO) * sizeof(uint32_t), device);
      P.ptab = (const uint32_t*)ptab.p;
      P.n_vals = nvals + KV_PTAB_PSEUDO;
    }
    {  // match tables: one allocation, three [word][entity] tables
      const PolicySet& pp = ps->ps;
      const Batch& bb = bt->b;
      P.mt_ns_words = (pp.n_nss_bits + 31) / 32;
      P.mt_ann_words = (pp.n_ann_bits + 31) / 32;
      P.mt_sel_words = (uint32_t)((pp.selectors.size() + 31) / 32);
      const size_t n_ns = (size_t)P.mt_ns_words * bb.nsms.size(), n_an = (size_t)P.mt_ann_words * bb.asets.size(),
                   n_sl = (size_t)P.mt_sel_words * bb.lsets.size();
      mtab.alloc(std::max<size_t>(n_ns + n_an + n_sl, 1) * sizeof(uint32_t), device);
      mt_ns = (uint32_t*)mtab.p;
      mt_ann = mt_ns + n_ns;
      mt_sel = mt_ann + n_an;
      P.mt_ns = mt_ns;
      P.mt_ann = mt_ann;
      mtbf.upload(mtab_bit_filters(pp), device);
      P.mt_bitf = (const uint32_t*)mtbf.p;
      P.mt_sel = mt_sel;
      mt_words = P.mt_ns_words + P.mt_ann_words + P.mt_sel_words;
      mt_entities = (uint32_t)std::max({bb.nsms.size(), bb.asets.size(), bb.lsets.size()});
    }
    if (dp.mtup_words) {  // match bits of every rule per match tuple: mtup_words per tuple
      mtup.alloc(std::max<size_t>((size_t)dp.mtup_words * bt->b.tup_rep.size(), 1) * sizeof(uint32_t), device);
      P.mtup = (const uint32_t*)mtup.p;
      P.mtup_words = dp.mtup_words;
      // factor tables [slot][entity] of the five entity types, one allocation
      const DevBatch& bv = *bhost;
      const uint32_t ne[KV_FAC_TYPES] = {bv.n_kent, bv.n_nsm, bv.n_asets, bv.n_lsets, bv.n_ns};
      uint64_t at = 0;
      for (uint32_t t = 0; t < KV_FAC_TYPES; t++) {
        P.fac_off[t] = at;
        at += (uint64_t)dp.fac_slots * ne[t];
        fac_entities = std::max(fac_entities, ne[t]);
      }
      ftab.alloc(std::max<uint64_t>(at, 1) * sizeof(uint32_t), device);
      P.fac_tab = (uint32_t*)ftab.p;
    }
    pview.upload_raw(&P, sizeof(DevPS), device);  // read through a uniform pointer (scalar loads)
    ptab_pipe = dp.specialized() && !(getenv("KVGPU_PTAB_PIPE") && getenv("KVGPU_PTAB_PIPE")[0] == '0');
    if (ptab_pipe) {  // the second set of per-pass tables
      if (dp.ptab_fn) {
        ptab1.alloc(ptab.n, device);
        P.ptab = (const uint32_t*)ptab1.p;
      }
      mtab1.alloc(mtab.n, device);
      mt1_ns = (uint32_t*)mtab1.p;
      mt1_ann = mt1_ns + (mt_ann - mt_ns);
      mt1_sel = mt1_ns + (mt_sel - mt_ns);
      P.mt_ns = mt1_ns;
      P.mt_ann = mt1_ann;
      P.mt_sel = mt1_sel;
      if (dp.mtup_words) {
        mtup1.alloc(mtup.n, device);
        P.mtup = (const uint32_t*)mtup1.p;
        ftab1.alloc(ftab.n, device);
        P.fac_tab = (uint32_t*)ftab1.p;
      }
      pview1.upload_raw(&P, sizeof(DevPS), device);
    }
    nrules = ps->ps.rules.size();
    nres = bt->b.res.size();
    ntup = (uint32_t)bt->b.tup_rep.size();
    O.full = 0;
    // the status matrix: asked for, or the bytecode engine's per-scope counts read it back
    // (the specialized kernels count scopes inside the pass, O.full bit 3)
    if ((mode & (KV_MODE_STATUS | KV_MODE_ERRORS)) || ((mode & KV_MODE_SCOPES) && !dp.specialized())) {
      st.alloc(nrules * nres, device);
      O.status = (uint8_t*)st.p;
      O.full |= 1;
      if (dp.specialized()) {  // (flags of every segment, set by each pass)
        sflag.alloc(std::max<uint64_t>(nrules * ((nres + KV_RWG - 1) / KV_RWG), 1), device);
        HIPCHK(hipMemset(sflag.p, 1, sflag.n));
        O.sflag = (uint8_t*)sflag.p;
      }
    }
    if (mode & KV_MODE_ERRORS) {
      er8.alloc(nrules * nres * sizeof(ErrRec8), device);
      O.err8 = (ErrRec8*)er8.p;
      O.err = nullptr;  // full records: allocated by fetch() for the re-run pass, if some record is wide
      O.full |= 2;
      if (dp.gs_groups) {  // 64 x members 16 B slots per wave and group, a count per (group, wave)
        const uint64_t nw = (nres + 63) / 64;
        gsite.alloc(std::max<uint64_t>((uint64_t)dp.gs_members * nw * 64u * 16u, 16), device);
        gcnt.alloc(std::max<uint64_t>((uint64_t)dp.gs_groups * nw * sizeof(uint32_t), 4), device);
        O.gsite = (uint32_t*)gsite.p;
        O.gcnt = (uint32_t*)gcnt.p;
      }
    }
    cn.alloc(std::max<uint64_t>(nrules, 1) * KV_HIST * sizeof(unsigned long long), device);
    O.counts = (unsigned long long*)cn.p;
    if (ptab_pipe) cn1.alloc(cn.n, device);
    if (mode & KV_MODE_SCOPES) {
      // scope of every resource = its namespace index in the batch namespace table
      std::vector<uint32_t> sc(nres);
      for (uint64_t i = 0; i < nres; i++) sc[i] = bt->b.res[i].ns_index;
      nscopes = (uint32_t)bt->b.namespaces.size();
      scope.upload(sc, device);
      scn.alloc(std::max<uint64_t>((uint64_t)nscopes * nrules, 1) * KV_HIST * sizeof(unsigned long long), device);
      if (ptab_pipe) scn1.alloc(scn.n, device);
      O.scope = (const uint32_t*)scope.p;
      O.scounts = (unsigned long long*)scn.p;
      if (dp.specialized()) O.full |= 8;
    }
    if (getenv("KVGPU_JIT_STAMPS") && dp.specialized()) {  // diagnostics: segment stamps of the rule kernels' waves
      const uint64_t n = (nres + KV_RWG - 1) / KV_RWG * KV_RWAVES * kJitStamps;
      stamps.alloc(std::max<uint64_t>(n, 1) * sizeof(unsigned long long), device);
      HIPCHK(hipMemset(stamps.p, 0, stamps.n));
      for (hipModule_t m : dp.mods) {  // the kernels' global kvj_stamps -> this buffer
        hipDeviceptr_t g = nullptr;
        size_t gs = 0;
        if (hipModuleGetGlobal(&g, &gs, m, "kvj_stamps") == hipSuccess && gs == sizeof(void*))
          HIPCHK(hipMemcpy(g, &stamps.p, sizeof(void*), hipMemcpyHostToDevice));
        else
          (void)hipGetLastError();
      }
    }
    stream = StreamPool::get().take(device, hipStreamDefault);
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    side = StreamPool::get().take(device, hipStreamNonBlocking);
    if (ptab_pipe) {
      pside = StreamPool::get().take(device, hipStreamNonBlocking, true);  // (the lowest priority)
      for (int b = 0; b < 2; b++) {
        HIPCHK(hipEventCreateWithFlags(&ev_pt[b], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev_rk[b], hipEventDisableTiming));
      }
    }
    HIPCHK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ev_rkf, hipEventDisableTiming));
    for (hipEvent_t& e : ev_rkj) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  // drop the kv_batch (parts sessions: the host batch is the caller's, and may be freed after
  // kv_session_attach_part); the session keeps the device copy through batch_ref, and so does
  // every other session using it (the batch's cache keeps its entry for later sessions)
  void detach_batch() { bt = nullptr; }
  // renumber the scope of every resource through map (batch namespace -> session scope) and
  // size the per-scope counts for n_total scopes
  void remap_scopes(const std::vector<uint32_t>& map, uint32_t n_total) {
    if (!(mode & KV_MODE_SCOPES)) return;
    HIPCHK(hipSetDevice(device));
    DevBuf m;
    m.upload(map, device);
    HIPCHK(launch_remap_u32((uint32_t*)scope.p, nres, (const uint32_t*)m.p, stream));
    HIPCHK(hipStreamSynchronize(stream));
    nscopes = n_total;
    scn.alloc(std::max<uint64_t>((uint64_t)nscopes * nrules, 1) * KV_HIST * sizeof(unsigned long long), device);
    if (ptab_pipe) scn1.alloc(scn.n, device);
    O.scounts = (unsigned long long*)scn.p;
  }
  ~DevSession() {
    (void)hipSetDevice(device);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (ev_rkf) (void)hipEventDestroy(ev_rkf);
    for (hipEvent_t e : ev_rkj)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : kev) (void)hipEventDestroy(e);
    for (hipStream_t x : rkx) StreamPool::get().give(device, hipStreamNonBlocking, x);
    for (int b = 0; b < 2; b++) {
      if (ev_pt[b]) (void)hipEventDestroy(ev_pt[b]);
      if (ev_rk[b]) (void)hipEventDestroy(ev_rk[b]);
    }
    StreamPool::get().give(device, hipStreamNonBlocking, pside, true);
    StreamPool::get().give(device, hipStreamNonBlocking, side);
    StreamPool::get().give(device, hipStreamDefault, stream);
  }
  // enqueue `iters` passes, wait, return HIP-event milliseconds of all passes
  // vm: run the passes on the bytecode engine even when the policy set has specialized kernels
  // (the full-record re-run of fetch: the specialized kernels write compact records only)
  double run(int iters, bool vm = false) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipEventRecord(e0, stream));
    const bool pipe = ptab_pipe && dps->specialized() && !vm && nres;
    if (pipe && iters > 0) {  // pass 0's tables, after the start event
      HIPCHK(hipStreamWaitEvent(pside, e0, 0));
      launch_tables(0);
    }
    for (int i = 0; i < iters; i++) {
      rec_compact = dps->specialized() && !vm;
      if (pipe) {  // tables and zeroed counts of set i & 1 from launch_tables
        const int b = i & 1;
        launch_specialized(b);
        if (O.full & 8u)
          HIPCHK(launch_scope_totals((const unsigned long long*)(b ? scn1.p : scn.p), nscopes, (uint32_t)nrules,
                                     (unsigned long long*)(b ? cn1.p : cn.p), stream));
        // set b's last readers (rule kernels) and writers (scope totals) are done after this event:
        // launch_tables(b) of pass i + 2 zeroes its counts behind it
        HIPCHK(hipEventRecord(ev_rk[b], stream));
        if (i + 1 < iters) {  // the next pass's tables, once pass i - 1's kernels are done with them
          const int nb = (i + 1) & 1;
          if (i >= 1) HIPCHK(hipStreamWaitEvent(pside, ev_rk[nb], 0));
          launch_tables(nb);
        }
        continue;
      }
      // the match tables on the side stream, forked from and joined back into `stream`
      // (specialized passes; the bytecode engine runs everything in order on `stream`)
      hipStream_t ms = rec_compact ? side : stream;
      if (rec_compact) {
        HIPCHK(hipEventRecord(ev_fork, stream));
        HIPCHK(hipStreamWaitEvent(side, ev_fork, 0));
      }
      HIPCHK(hipMemsetAsync(cn.p, 0, cn.n, ms));
      if (mode & KV_MODE_SCOPES) HIPCHK(hipMemsetAsync(scn.p, 0, scn.n, ms));
      HIPCHK(launch_mtab((const DevPS*)pview.p, bview, mt_words, mt_entities, mt_ns, mt_ann, mt_sel, ms));
      if (rec_compact) {
        launch_specialized();  // (per-scope counts inside the rule kernels)
        if (O.full & 8u)  // per-rule totals from the per-scope counts (the kernels add only those)
          HIPCHK(launch_scope_totals((const unsigned long long*)scn.p, nscopes, (uint32_t)nrules,
                                     (unsigned long long*)cn.p, stream));
      } else {
        DevOut Ov = O;
        Ov.full &= ~8u;
        HIPCHK(launch_validate((const DevPS*)pview.p, bview, (uint32_t)nres, Ov, 0, (uint32_t)nrules, stream));
        if (mode & KV_MODE_SCOPES)
          HIPCHK(launch_scope_counts(O.status, (const uint32_t*)scope.p, (uint32_t)nres, (uint32_t)nrules, nscopes,
                                     (unsigned long long*)scn.p, stream));
      }
    }
    HIPCHK(hipEventRecord(e1, stream));
    HIPCHK(hipEventSynchronize(e1));
    order_kernels();
    if (pipe && iters > 0 && ((iters - 1) & 1)) {  // the last pass counted into set 1: it becomes set 0
      cn.swap(cn1);
      scn.swap(scn1);
      O.counts = (unsigned long long*)cn.p;
      if (mode & KV_MODE_SCOPES) O.scounts = (unsigned long long*)scn.p;
    }
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, e0, e1));
    if (stamps.p) report_stamps();
    return t;
  }
  // mean shader cycles per wave between consecutive stamps of the last rule kernel (segment k: from
  // stamp k - 1 to stamp k), and the mean wave lifetime
  void report_stamps() {
    std::vector<unsigned long long> h(stamps.n / sizeof(unsigned long long));
    HIPCHK(hipMemcpy(h.data(), stamps.p, stamps.n, hipMemcpyDeviceToHost));
    double seg[kJitStamps] = {}, life = 0;
    uint64_t n[kJitStamps] = {}, nl = 0;
    for (size_t w = 0; w + kJitStamps <= h.size(); w += kJitStamps) {
      const unsigned long long* x = &h[w];
      uint32_t last = 0;
      for (uint32_t k = 1; k < kJitStamps; k++)
        if (x[k] && x[last]) {
          seg[k] += (double)(x[k] - x[last]);
          n[k]++;
          last = k;
        }
      if (x[0] && x[last] && last) {
        life += (double)(x[last] - x[0]);
        nl++;
      }
    }
    fprintf(stderr, "[kvgpu] stamps: wave lifetime %.0f cycles;", nl ? life / nl : 0.0);
    for (uint32_t k = 1; k < kJitStamps; k++)
      if (n[k]) fprintf(stderr, " seg%u %.0f", k, seg[k] / n[k]);
    fprintf(stderr, "\n");
  }
  // one launch per rule kernel of the specialized kernels, 256 resources per workgroup
  // the per-pass tables of set b (match tables, factored match, value-predicate table) of a
  // pipelined pass, on `pside`, then their event
  void launch_tables(int b) {
    const DevPS* P = (const DevPS*)(b ? pview1.p : pview.p);
    DevBuf& c = b ? cn1 : cn;
    HIPCHK(hipMemsetAsync(c.p, 0, c.n, pside));
    if (mode & KV_MODE_SCOPES) {
      DevBuf& sc = b ? scn1 : scn;
      HIPCHK(hipMemsetAsync(sc.p, 0, sc.n, pside));
    }
    HIPCHK(launch_mtab(P, bview, mt_words, mt_entities, b ? mt1_ns : mt_ns, b ? mt1_ann : mt_ann, b ? mt1_sel : mt_sel,
                       pside));
    if (dps->mtup_words && ntup)
      HIPCHK(launch_mfac(P, bview, dps->fac_slots, fac_entities, dps->mtup_words, ntup,
                         (uint32_t*)(b ? mtup1.p : mtup.p), pside));
    if (dps->ptab_fn) {
      const Val* V = bhost->vals;
      const uint8_t* S = bhost->bstr;
      uint32_t NV = nvals;
      uint32_t* PT = (uint32_t*)(b ? ptab1.p : ptab.p);
      void* targs[] = {(void*)&P, (void*)&V, (void*)&S, (void*)&NV, (void*)&PT};
      HIPCHK(hipModuleLaunchKernel(dps->ptab_fn, (NV + KV_PTAB_PSEUDO + KV_WG - 1) / KV_WG, dps->ptab_rows, 1, KV_WG, 1, 1,
                                   0, pside, targs, nullptr));
    }
    HIPCHK(hipEventRecord(ev_pt[b], pside));
  }
  // pb: the pipelined table this pass reads (launch_ptab), -1: build the table here
  void launch_specialized(int pb = -1) {
    if (nres == 0) {  // (join the side stream's table work all the same)
      HIPCHK(hipEventRecord(ev_join, side));
      HIPCHK(hipStreamWaitEvent(stream, ev_join, 0));
      return;
    }
    const uint32_t blocks = (uint32_t)((nres + KV_RWG - 1) / KV_RWG);
    const DevPS* P = (const DevPS*)(pb == 1 ? pview1.p : pview.p);
    const Node* N = bhost->nodes;
    const Val* V = bhost->vals;
    const uint8_t* S = bhost->bstr;
    if (pb >= 0) {
      HIPCHK(hipStreamWaitEvent(stream, ev_pt[pb], 0));
    } else {
    if (dps->ptab_fn) {  // every leaf predicate once per distinct value (+ pseudo columns), before the rule kernels
      uint32_t NV = nvals;
      uint32_t* PT = (uint32_t*)ptab.p;
      void* targs[] = {(void*)&P, (void*)&V, (void*)&S, (void*)&NV, (void*)&PT};
      HIPCHK(hipModuleLaunchKernel(dps->ptab_fn, (NV + KV_PTAB_PSEUDO + KV_WG - 1) / KV_WG, dps->ptab_rows, 1, KV_WG, 1, 1, 0,
                                   stream, targs, nullptr));
    }
    if (dps->mtup_words && ntup)  // every rule's match bit per tuple (after kv_mtab, on the side stream)
      HIPCHK(launch_mfac(P, bview, dps->fac_slots, fac_entities, dps->mtup_words, ntup, (uint32_t*)mtup.p, side));
    HIPCHK(hipEventRecord(ev_join, side));
    HIPCHK(hipStreamWaitEvent(stream, ev_join, 0));
    }
    DevOut Ov = O;
    if (pb == 1) {  // counts of set 1
      Ov.counts = (unsigned long long*)cn1.p;
      if (mode & KV_MODE_SCOPES) Ov.scounts = (unsigned long long*)scn1.p;
    }
    uint32_t r0 = 0;
    void* args[] = {(void*)&P, (void*)&bview, (void*)&N, (void*)&V, (void*)&S, (void*)&Ov, (void*)&r0};
    // Rule kernels of a pass (they write disjoint rule rows): three or more are dealt round-robin
    // over `stream`, `side` and a third stream, forked from and joined back into `stream`, so a
    // kernel's last workgroups share the chip with the next kernels' first instead of draining it;
    // once a pass has timed them, they go longest first (and two kernels then go over two
    // streams: the short one fills the long one's tail). C3 (17 kernels), ms per pass on one box:
    // one stream 3.56, two 2.96-3.01, three 2.66-2.69, four 2.73-2.75 (a process has 4 hardware
    // queues; the pipeline stream takes one). C4 (2 kernels, 150 and 515 us): one stream 0.690,
    // two in plan order 0.713-0.714, two longest first 0.613-0.617.
    constexpr uint32_t kRuleStreams = 3;
    const std::vector<hipFunction_t>& fs = dps->fns_for(Ov.full);
    const uint32_t nk = (uint32_t)fs.size();
    if (korder.empty() && nk > 1) {
      std::lock_guard<std::mutex> g(dps->order_mu);
      if (dps->korder.size() == nk) korder = dps->korder;
    }
    const bool ordered = korder.size() == nk && nk > 1;
    const uint32_t ns = nk >= 3 ? std::min<uint32_t>(kRuleStreams, nk) : (ordered ? nk : 1u);
    // the first pass of a session with 2+ kernels times them (events around each launch)
    const bool timing = !ordered && nk > 1 && !ktiming;
    if (timing) {
      while (kev.size() < 2 * nk) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        kev.push_back(e);
      }
      ktiming = true;
    }
    while (rkx.size() + 2 < ns) rkx.push_back(StreamPool::get().take(device, hipStreamNonBlocking));
    hipStream_t sts[4] = {stream, side, rkx.size() > 0 ? rkx[0] : nullptr, rkx.size() > 1 ? rkx[1] : nullptr};
    if (ns > 1) {
      HIPCHK(hipEventRecord(ev_rkf, stream));
      for (uint32_t q = 1; q < ns; q++) HIPCHK(hipStreamWaitEvent(sts[q], ev_rkf, 0));
    }
    for (uint32_t k = 0; k < nk; k++) {
      const uint32_t f = ordered ? korder[k] : k;
      hipStream_t st = sts[k % ns];
      if (timing) HIPCHK(hipEventRecord(kev[2 * f], st));
      HIPCHK(hipModuleLaunchKernel(fs[f], blocks, 1, 1, KV_RWG, 1, 1, 0, st, args, nullptr));
      if (timing) HIPCHK(hipEventRecord(kev[2 * f + 1], st));
    }
    for (uint32_t q = 1; q < ns; q++) {
      HIPCHK(hipEventRecord(ev_rkj[q - 1], sts[q]));
      HIPCHK(hipStreamWaitEvent(stream, ev_rkj[q - 1], 0));
    }
  }
  // after a timed pass has completed: the rule kernels' launch order, longest first
  void order_kernels() {
    if (!ktiming || !korder.empty()) return;
    const uint32_t nk = (uint32_t)(kev.size() / 2);
    std::vector<std::pair<float, uint32_t>> d(nk);
    for (uint32_t k = 0; k < nk; k++) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, kev[2 * k], kev[2 * k + 1]) != hipSuccess) {
        (void)hipGetLastError();
        return;  // (not timed in this run: keep the plan order)
      }
      d[k] = {ms, k};
    }
    std::stable_sort(d.begin(), d.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    for (const auto& x : d) korder.push_back(x.second);
    std::lock_guard<std::mutex> g(dps->order_mu);
    if (dps->korder.empty()) dps->korder = korder;
  }
  // status-matrix bytes the last pass wrote: the (rule, workgroup) segments whose flag it set (a
  // segment left unwritten is all NOMATCH and filled at fetch), or the whole matrix without flags
  uint64_t written_status_bytes() {
    if (!O.status) return 0;
    if (!O.sflag || !dps->specialized()) return nrules * nres;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(stream));
    std::vector<uint8_t> f(sflag.n);
    if (!f.empty()) HIPCHK(hipMemcpy(f.data(), sflag.p, f.size(), hipMemcpyDeviceToHost));
    const uint64_t nwg = (nres + KV_RWG - 1) / KV_RWG, last = nres - (nwg - 1) * KV_RWG;
    uint64_t bytes = 0;
    for (uint64_t i = 0; i < nrules * nwg && i < f.size(); i++)
      if (f[i]) bytes += (i % nwg == nwg - 1) ? last : KV_RWG;
    return bytes;
  }
  std::vector<int64_t> read_counts() {
    HIPCHK(hipSetDevice(device));
    std::vector<unsigned long long> c(nrules * KV_HIST);
    if (!c.empty()) HIPCHK(hipMemcpy(c.data(), cn.p, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return std::vector<int64_t>(c.begin(), c.end());
  }
  std::vector<int64_t> read_scope_counts() {
    HIPCHK(hipSetDevice(device));
    std::vector<unsigned long long> c((size_t)nscopes * nrules * KV_HIST);
    if (!c.empty()) HIPCHK(hipMemcpy(c.data(), scn.p, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return std::vector<int64_t>(c.begin(), c.end());
  }
  // statuses into rows [rule][lo, lo + nres) of the result's [rule][n_total] matrix, and
  // the compacted error records of this shard
  void fetch(kv_result* out, ResultPart* part, uint64_t lo, uint64_t n_total) {
    HIPCHK(hipSetDevice(device));
    const bool verbose = getenv("KVGPU_VERBOSE") != nullptr;
    auto tl = std::chrono::steady_clock::now();
    // phase boundary: the stream drained, the time since the last one into the result's phases
    // (the first part's, so parts on several devices do not add up)
    auto lap = [&](const char* what) {
      HIPCHK(hipStreamSynchronize(stream));
      const auto now = std::chrono::steady_clock::now();
      const double ms = std::chrono::duration<double, std::milli>(now - tl).count();
      tl = now;
      if (part == &out->parts[0]) out->phases.push_back({what, ms});
      if (verbose) fprintf(stderr, "[kvgpu] fetch: %s %.1f ms\n", what, ms);
    };
    const bool want_st = O.status && (mode & (KV_MODE_STATUS | KV_MODE_ERRORS)) && nres && nrules;
    bool side_copy = false;
    uint64_t spack_bytes = 0;
    // A permuted batch fetched whole comes back in the caller's order: the statuses are gathered on
    // the device (stc[rule][j] = st[rule][store index of j]) and the records scattered to the
    // caller's (rule, resource) order, so one status matrix crosses PCIe and the host permutes
    // nothing. Its copy runs on the side stream, beside the record kernels.
    // Specialized passes: the statuses cross in the transfer form (the segments the pass wrote, 4
    // bits a status; C3: 0.48 GB for a 2.47 GB matrix) and the host materialises the matrix when an
    // accessor reads it; records then stay in store order
    const bool packed = want_st && out->sparse;
    if (packed) {
      const uint64_t nwg = (nres + KV_RWG - 1) / KV_RWG, nch = (nwg + KV_WG - 1) / KV_WG;
      if (s_ccnt.n < nrules * nch * sizeof(uint32_t)) {
        s_ccnt.alloc(nrules * nch * sizeof(uint32_t), device);
        s_cbase.alloc(nrules * nch * sizeof(unsigned long long), device);
      }
      HIPCHK(launch_status_pack(O.status, O.sflag, (uint32_t)nres, (uint32_t)nrules, nullptr, (uint32_t*)s_ccnt.p,
                                nullptr, stream));
      std::vector<uint32_t> cc(nrules * nch);
      std::vector<unsigned long long> cb(nrules * nch);
      HIPCHK(hipMemcpyAsync(cc.data(), s_ccnt.p, cc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      part->nwg = nwg;
      part->sbase.resize(nrules);
      unsigned long long t = 0;
      for (size_t i = 0; i < cc.size(); i++) {
        if (i % nch == 0) part->sbase[i / nch] = t;
        cb[i] = t;
        t += cc[i];
      }
      const uint64_t bytes = t * (KV_RWG / 2);
      if (s_pack.n < std::max<uint64_t>(bytes, 1)) s_pack.alloc(std::max<uint64_t>(bytes, 1), device);
      HIPCHK(hipMemcpyAsync(s_cbase.p, cb.data(), cb.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
      HIPCHK(launch_status_pack(O.status, O.sflag, (uint32_t)nres, (uint32_t)nrules,
                                (const unsigned long long*)s_cbase.p, nullptr, (uint8_t*)s_pack.p, stream));
      part->sflag.alloc(nrules * nwg);
      part->spack.alloc(bytes);
      // copied after the records: the record steps' small copies (offsets, flags, code tables)
      // would otherwise queue behind these bytes on the copy engines at every host round trip
      spack_bytes = bytes;
      lap("status_pack");
    }
    bool caller = !packed && want_st && bt && lo == 0 && nres == n_total && !bt->b.order.empty();
    if (caller && !stc.p) {  // the gathered copy is a second status matrix: only with room to spare
      size_t fr = 0, tot = 0;
      if (hipMemGetInfo(&fr, &tot) != hipSuccess) caller = false;
      fr += dev_pool_held(device);  // (kept buffers are freed when an allocation needs them)
      if (fr < nrules * nres + nres * 8u + (512ull << 20)) caller = false;
    }
    if (caller) {
      if (!inv_d.p) inv_d.upload_raw(bt->inverse(), nres * sizeof(uint32_t), device);
      if (!stc.p) stc.alloc(nrules * nres, device);
      HIPCHK(launch_gather_rows((const uint8_t*)st.p, (const uint32_t*)inv_d.p, nrules, nres, (uint8_t*)stc.p, stream));
      HIPCHK(hipEventRecord(ev_fork, stream));
      HIPCHK(hipStreamWaitEvent(side, ev_fork, 0));
      HIPCHK(hipMemcpyAsync(out->status.data(), stc.p, nrules * nres, hipMemcpyDeviceToHost, side));
      side_copy = true;
      out->caller_order = true;
      lap("status_gather");
    } else if (want_st && !packed) {
      HIPCHK(hipMemcpy2DAsync(out->status.data() + lo, n_total, st.p, nres, nres, nrules, hipMemcpyDeviceToHost,
                              stream));
      lap("status_d2h");
    }
    if (O.err8 && nres && nrules) {
      const uint32_t tiles = (uint32_t)((nres + KV_WG - 1) / KV_WG);
      part->tiles = tiles;
      if (!r_offs.p) {
        r_offs.alloc((size_t)nrules * tiles * sizeof(uint32_t), device);
        r_tot.alloc(nrules * sizeof(unsigned long long), device);
        r_base.alloc((nrules + 1) * sizeof(unsigned long long), device);
        r_wide.alloc(sizeof(uint32_t), device);
      }
      const uint32_t* ord = nullptr;
      unsigned long long* masks = nullptr;
      if (caller) {  // record ranks over the caller-order statuses
        if (!ord_d.p) ord_d.upload_raw(bt->b.order.data(), nres * sizeof(uint32_t), device);
        if (!r_mask.p) r_mask.alloc((size_t)nrules * tiles * (KV_WG / 64) * sizeof(unsigned long long), device);
        ord = (const uint32_t*)ord_d.p;
        masks = (unsigned long long*)r_mask.p;
      }
      const uint8_t* rank_st = caller ? (const uint8_t*)stc.p : O.status;
      // a specialized pass's unwritten segments hold no records: the record kernels skip them
      // (their statuses are neither filled nor read)
      const uint8_t* seg_flags = rec_compact && !caller ? O.sflag : nullptr;
      HIPCHK(launch_rec_compact(rank_st, O.err8, nullptr, (uint32_t)nres, (uint32_t)nrules, (uint32_t*)r_offs.p,
                                (unsigned long long*)r_tot.p, (unsigned long long*)r_base.p, nullptr, nullptr, nullptr,
                                0, rec_compact ? (const uint8_t*)dps->rcompact.p : nullptr, nullptr, masks, seg_flags,
                                stream));
      // the fetch's small device-to-host copies go through one page-locked staging block (a copy
      // into pageable memory is staged by the runtime and waited for behind the DMA queue)
      const size_t tb = (size_t)nrules * KV_REC_CODES, sb = ((nrules + 1) * 8 + 63) & ~(size_t)63;
      if (hstage.size() < sb + nrules * 4 + 64 + tb * 8) hstage.alloc(sb + nrules * 4 + 64 + tb * 8);
      part->base.resize(nrules + 1);
      part->offs.alloc((size_t)nrules * tiles);
      HIPCHK(hipMemcpyAsync(hstage.data(), r_base.p, part->base.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(part->offs.data(), r_offs.p, part->offs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost,
                            stream));
      lap("records_count");
      memcpy(part->base.data(), hstage.data(), part->base.size() * sizeof(uint64_t));
      const uint64_t total = part->base[nrules];
      if (r_out8.n < total * sizeof(ErrRec8)) {
        r_out8.alloc(std::max<uint64_t>(total, 1) * sizeof(ErrRec8), device);
        lap("records_alloc");
      }
      HIPCHK(hipMemsetAsync(r_wide.p, 0, sizeof(uint32_t), stream));
      if (rec_compact && O.gsite) {  // the groups' site records to their members' slots
        HIPCHK(launch_gsite_expand(O.gsite, O.gcnt, (const GSiteDesc*)dps->gsdesc.p, (const uint32_t*)dps->gsmem.p,
                                   dps->gs_groups, (uint32_t)nres, O.err8, stream));
        lap("records_expand");
      }
      HIPCHK(launch_rec_compact(O.status, O.err8, nullptr, (uint32_t)nres, (uint32_t)nrules, (uint32_t*)r_offs.p,
                                nullptr, (unsigned long long*)r_base.p, (ErrRec8*)r_out8.p, nullptr,
                                (uint32_t*)r_wide.p, 1, rec_compact ? (const uint8_t*)dps->rcompact.p : nullptr, ord,
                                masks, seg_flags, stream));
      HIPCHK(hipMemcpyAsync(hstage.data() + sb, r_wide.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      lap("records_scatter");
      uint32_t wide = 0;
      memcpy(&wide, hstage.data() + sb, sizeof(uint32_t));
      // Record codes: a rule's records cross PCIe as 1-byte codes into a table of its distinct
      // records (C2: 206 MB of 8-byte records -> 26 MB of codes, C3: 3.6 GB -> 0.45 GB); skipped
      // when some record is wide (the full records of the re-run below are kept parallel to every
      // compact record)
      const ErrRec8* src = (const ErrRec8*)r_out8.p;
      uint64_t keep = total;
      bool coded = false;
      part->raw.clear();
      if (!wide && total && nrules) {
        if (r_tkey.n < tb * sizeof(unsigned long long)) {
          r_tkey.alloc(tb * sizeof(unsigned long long), device);
          r_raw.alloc(nrules * sizeof(uint32_t), device);
          r_nbase.alloc(nrules * sizeof(unsigned long long), device);
        }
        if (r_code.n < total) r_code.alloc(total, device);
        HIPCHK(hipMemsetAsync(r_tkey.p, 0xFF, tb * sizeof(unsigned long long), stream));
        HIPCHK(hipMemsetAsync(r_raw.p, 0, nrules * sizeof(uint32_t), stream));
        HIPCHK(launch_rec_codes((const ErrRec8*)r_out8.p, (const unsigned long long*)r_base.p, (uint32_t)nrules,
                                (unsigned long long*)r_tkey.p, (uint8_t*)r_code.p, (uint32_t*)r_raw.p, nullptr, nullptr,
                                0, stream));
        const uint32_t* rawf = (const uint32_t*)hstage.data();
        const unsigned long long* keys = (const unsigned long long*)(hstage.data() + ((nrules * 4 + 63) & ~(size_t)63));
        HIPCHK(hipMemcpyAsync((void*)rawf, r_raw.p, nrules * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync((void*)keys, r_tkey.p, tb * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        part->raw.assign(nrules, 0);
        part->nbase.assign(nrules, 0);
        part->tab.assign(tb, ErrRec8{0u, 0u});
        keep = 0;
        for (uint64_t q = 0; q < nrules; q++) {
          part->raw[q] = rawf[q] ? 1 : 0;
          part->nbase[q] = keep;
          if (rawf[q]) keep += part->base[q + 1] - part->base[q];
        }
        for (size_t t = 0; t < tb; t++)
          if (keys[t] != ~0ull) part->tab[t] = ErrRec8{(uint32_t)(keys[t] >> 32), (uint32_t)keys[t]};
        if (keep) {
          if (r_out8b.n < keep * sizeof(ErrRec8)) r_out8b.alloc(keep * sizeof(ErrRec8), device);
          HIPCHK(hipMemcpyAsync(r_nbase.p, part->nbase.data(), nrules * sizeof(unsigned long long),
                                hipMemcpyHostToDevice, stream));
          HIPCHK(launch_rec_codes((const ErrRec8*)r_out8.p, (const unsigned long long*)r_base.p, (uint32_t)nrules,
                                  nullptr, nullptr, (uint32_t*)r_raw.p, (const unsigned long long*)r_nbase.p,
                                  (ErrRec8*)r_out8b.p, 1, stream));
          src = (const ErrRec8*)r_out8b.p;
        }
        coded = true;
        lap("records_code");
      }
      const auto th0 = std::chrono::steady_clock::now();
      part->rec.alloc(keep);
      if (part == &out->parts[0])
        out->phases.push_back(
            {"host_alloc", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count()});
      if (coded) part->code.alloc(total);
      tl = std::chrono::steady_clock::now();
      if (keep) HIPCHK(hipMemcpyAsync(part->rec.data(), src, keep * sizeof(ErrRec8), hipMemcpyDeviceToHost, stream));
      if (coded) HIPCHK(hipMemcpyAsync(part->code.data(), r_code.p, total, hipMemcpyDeviceToHost, stream));
      lap("records_d2h");
      if (wide) {  // re-run the pass once writing full records (same statuses), compact those too
        if (!er.p) er.alloc(nrules * nres * sizeof(ErrRec), device);
        O.err = (ErrRec*)er.p;
        O.full |= 4;
        run(1, true);
        O.full &= ~4u;
        if (r_outw.n < total * sizeof(ErrRec)) r_outw.alloc(std::max<uint64_t>(total, 1) * sizeof(ErrRec), device);
        HIPCHK(launch_rec_compact(O.status, O.err8, O.err, (uint32_t)nres, (uint32_t)nrules, (uint32_t*)r_offs.p,
                                  nullptr, (unsigned long long*)r_base.p, (ErrRec8*)r_out8.p, (ErrRec*)r_outw.p,
                                  (uint32_t*)r_wide.p, 1, nullptr, ord, masks, nullptr, stream));
        part->recw.alloc(total);
        HIPCHK(hipMemcpyAsync(part->recw.data(), r_outw.p, total * sizeof(ErrRec), hipMemcpyDeviceToHost, stream));
        lap("records_wide_rerun");
      }
    }
    // pattern sets of foreach rules: per (pattern set, resource) the reduction key and the deciding
    // element's record, as the batch's fold left them (kvforeach.h)
    if (want_st && !ps->ps.fpats.empty() && batch_ref && batch_ref->ferec.p) {
      const std::vector<uint32_t>& fp = ps->ps.fpats;
      part->fe_key.alloc(fp.size() * nres);
      part->fe_rec.alloc(fp.size() * nres);
      for (size_t k = 0; k < fp.size(); k++)
        HIPCHK(hipMemcpyAsync(part->fe_key.data() + k * nres, (const uint32_t*)batch_ref->feacc.p + (size_t)fp[k] * nres,
                              nres * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(part->fe_rec.data(), batch_ref->ferec.p, fp.size() * nres * sizeof(ErrRec8),
                            hipMemcpyDeviceToHost, stream));
      lap("foreach_rows_d2h");
    }
    // any sets of foreach rules: per (any set, resource) the reduction key and the deciding
    // element's code word, per (alternative, resource) that element's record (kvforeach.h)
    if (want_st && !ps->ps.fanys.empty() && batch_ref && batch_ref->fearec.p) {
      const std::vector<uint32_t>& fa = ps->ps.fanys;
      size_t n_alts = 0;
      for (uint32_t fs : fa) n_alts += ps->ps.fsets[fs].alt_prog.size();
      part->fe_akey.alloc(fa.size() * nres);
      part->fe_acode.alloc(fa.size() * nres);
      part->fe_arec.alloc(n_alts * nres);
      for (size_t k = 0; k < fa.size(); k++)
        HIPCHK(hipMemcpyAsync(part->fe_akey.data() + k * nres, (const uint32_t*)batch_ref->feacc.p + (size_t)fa[k] * nres,
                              nres * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(part->fe_acode.data(), batch_ref->feacode.p, fa.size() * nres * sizeof(uint32_t),
                            hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(part->fe_arec.data(), batch_ref->fearec.p, n_alts * nres * sizeof(ErrRec8),
                            hipMemcpyDeviceToHost, stream));
      lap("foreach_any_rows_d2h");
    }
    // rules of several entries: the chain key per (chain, resource) (kvforeach.h kv_fe_chain)
    if (want_st && !ps->ps.fe_chains.empty() && batch_ref && batch_ref->feckey.p) {
      part->fe_ckey.alloc(ps->ps.fe_chains.size() * nres);
      HIPCHK(hipMemcpyAsync(part->fe_ckey.data(), batch_ref->feckey.p, ps->ps.fe_chains.size() * nres * sizeof(uint32_t),
                            hipMemcpyDeviceToHost, stream));
      lap("foreach_chain_d2h");
    }
    if (packed) {  // the statuses' transfer form (kv_status_pack_kernel above; the re-run leaves it)
      HIPCHK(hipMemcpyAsync(part->sflag.data(), O.sflag, part->sflag.size(), hipMemcpyDeviceToHost, stream));
      if (spack_bytes) HIPCHK(hipMemcpyAsync(part->spack.data(), s_pack.p, spack_bytes, hipMemcpyDeviceToHost, stream));
      lap("status_d2h");
    }
    HIPCHK(hipStreamSynchronize(stream));
    if (side_copy) {
      HIPCHK(hipStreamSynchronize(side));
      lap("status_d2h_wait");
    }
  }
};

// Sessions on the devices of a mask: contiguous resource shards, one host thread
// + HIP stream per part, policy set replicated, per-rule (and per-scope) counts
// summed over the parts by one RCCL all-reduce (distinct devices) when read.
struct SessionSet {
  kv_policyset* ps = nullptr;
  kv_batch* bt = nullptr;
  uint32_t mode = 0;
  uint64_t nrules = 0, nres = 0;
  std::vector<std::shared_ptr<kv_batch>> shards;           // empty: one part over the whole batch
  std::vector<std::pair<uint64_t, uint64_t>> ranges;       // resource range of each part
  std::vector<std::unique_ptr<DevSession>> parts;
  std::vector<ncclComm_t> comms;                           // one per part (distinct devices only)
  bool reduced = false;
  std::vector<int64_t> counts_, scope_counts_;
  std::vector<double> part_ms;                             // HIP-event ms of each part's last run
  // parts session (kv_session_create_parts): one caller batch per part, attached one by one;
  // scopes = the sorted union of the parts' namespaces, set when the last part is attached
  bool parts_mode = false, finalized = true;
  std::string ctx;
  std::vector<int> devs;
  std::vector<std::vector<std::string>> part_ns;
  std::vector<std::string> scope_names;

  // parts session: n empty parts (kv_session_attach_part fills them)
  SessionSet(kv_policyset* p, const char* ctx_json, uint32_t m, uint32_t n)
      : ps(p), mode(m), parts_mode(true), finalized(false), ctx(ctx_json ? ctx_json : "") {
    nrules = ps->ps.rules.size();
    parts.resize(n);
    ranges.assign(n, {0, 0});
    devs.assign(n, -1);
    part_ns.resize(n);
  }
  // part k = batch b on device d: uploaded, its device copy detached from the caller's batch
  void attach(uint32_t k, kv_batch* b, int d) {
    if (!parts_mode || finalized) throw std::runtime_error("not an open parts session");
    if (k >= parts.size()) throw std::runtime_error("part index out of range");
    if (parts[k]) throw std::runtime_error("part already attached");
    auto ds = std::make_unique<DevSession>(ps, b, ctx.empty() ? nullptr : ctx.c_str(), d, mode);
    part_ns[k] = b->b.namespaces;
    ds->detach_batch();
    parts[k] = std::move(ds);
    devs[k] = d;
    for (auto& q : parts)
      if (!q) return;
    finalize();
  }
  void finalize() {
    uint64_t at = 0;
    for (size_t k = 0; k < parts.size(); k++) {
      ranges[k] = {at, at + parts[k]->nres};
      at += parts[k]->nres;
    }
    nres = at;
    std::vector<std::string> all;
    for (auto& v : part_ns) all.insert(all.end(), v.begin(), v.end());
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    scope_names = all;
    for (size_t k = 0; k < parts.size(); k++) {
      std::vector<uint32_t> map(part_ns[k].size());
      for (size_t i = 0; i < map.size(); i++)
        map[i] = (uint32_t)(std::lower_bound(all.begin(), all.end(), part_ns[k][i]) - all.begin());
      parts[k]->remap_scopes(map, (uint32_t)all.size());
    }
    init_comms(devs);
    finalized = true;
  }
  void init_comms(const std::vector<int>& devices) {
    std::vector<int> uniq(devices);
    std::sort(uniq.begin(), uniq.end());
    if (devices.size() > 1 && std::unique(uniq.begin(), uniq.end()) == uniq.end()) {  // one rank per device
      comms.resize(devices.size());
      if (ncclCommInitAll(comms.data(), (int)devices.size(), devices.data()) != ncclSuccess) {
        comms.clear();
        throw HipError("ncclCommInitAll failed");
      }
    }
  }
  void check_ready() const {
    if (!finalized) throw std::runtime_error("parts session: not every part is attached");
  }
  int rccl_ranks() const {
    if (comms.empty()) return 0;
    int n = 0;
    if (ncclCommCount(comms[0], &n) != ncclSuccess) return -1;
    return n;
  }

  SessionSet(kv_policyset* p, kv_batch* b, const char* ctx_json, const std::vector<int>& devices, uint32_t m)
      : ps(p), bt(b), mode(m) {
    nrules = ps->ps.rules.size();
    nres = bt->b.res.size();
    if (devices.size() == 1) {
      ranges.push_back({0, nres});
      parts.push_back(std::make_unique<DevSession>(ps, bt, ctx_json, devices[0], mode));
      // KVGPU_RCCL_ALWAYS=1: reduce through a one-rank communicator too (exercises RCCL on one GPU)
      if (getenv("KVGPU_RCCL_ALWAYS") && getenv("KVGPU_RCCL_ALWAYS")[0] == '1') {
        comms.resize(1);
        if (ncclCommInitAll(comms.data(), 1, devices.data()) != ncclSuccess) {
          comms.clear();
          throw HipError("ncclCommInitAll failed");
        }
      }
      return;
    }
    ranges = shard_ranges(nres, (uint32_t)devices.size());
    shards.resize(devices.size());
    std::vector<std::thread> th;
    std::vector<std::string> errs(devices.size());
    for (size_t k = 0; k < devices.size(); k++)
      th.emplace_back([&, k]() {
        try {
          auto sb = std::make_shared<kv_batch>();
          sb->owner = ps;
          make_shard(bt->b, ranges[k].first, ranges[k].second, &sb->b);
          shards[k] = sb;
        } catch (const std::exception& e) {
          errs[k] = e.what();
        }
      });
    for (auto& t : th) t.join();
    for (auto& e : errs)
      if (!e.empty()) throw std::runtime_error(e);
    parts.resize(devices.size());
    th.clear();
    for (size_t k = 0; k < devices.size(); k++)
      th.emplace_back([&, k]() {
        try {
          parts[k] = std::make_unique<DevSession>(ps, shards[k].get(), ctx_json, devices[k], mode);
        } catch (const std::exception& e) {
          errs[k] = e.what();
        }
      });
    for (auto& t : th) t.join();
    for (auto& e : errs)
      if (!e.empty()) throw HipError(e);
    init_comms(devices);  // RCCL needs one rank per device
  }
  ~SessionSet() {
    for (ncclComm_t c : comms) (void)ncclCommDestroy(c);
  }
  template <class F>
  void each(F f) {
    if (parts.size() == 1) {
      f(0);
      return;
    }
    std::vector<std::thread> th;
    std::vector<std::string> errs(parts.size());
    for (size_t k = 0; k < parts.size(); k++)
      th.emplace_back([&, k]() {
        try {
          f(k);
        } catch (const std::exception& e) {
          errs[k] = e.what();
        }
      });
    for (auto& t : th) t.join();
    for (auto& e : errs)
      if (!e.empty()) throw HipError(e);
  }
  // `iters` passes on every part concurrently; the slowest part's HIP-event time
  double run(int iters) {
    check_ready();
    std::vector<double> ms(parts.size(), 0.0);
    each([&](size_t k) { ms[k] = parts[k]->run(iters); });
    reduced = false;
    part_ms = ms;
    return *std::max_element(ms.begin(), ms.end());
  }
  // a failed collective leaves ranks waiting: abort every communicator, never reuse them
  [[noreturn]] void abort_comms(const std::string& what) {
    for (ncclComm_t c : comms) (void)ncclCommAbort(c);
    comms.clear();
    comms_failed = true;
    throw HipError(what);
  }
  bool comms_failed = false;
  // counts of the last pass summed over the parts: RCCL all-reduce (ncclUint64, sum)
  // of the device count arrays across distinct devices, else a host sum
  void reduce() {
    check_ready();
    if (comms_failed) throw HipError("RCCL communicators were aborted after a failed all-reduce");
    if (reduced) return;
    counts_.assign(nrules * KV_HIST, 0);
    scope_counts_.clear();
    const bool scopes = (mode & KV_MODE_SCOPES) != 0;
    if (!comms.empty()) {
      if (ncclGroupStart() != ncclSuccess) abort_comms("ncclGroupStart failed");
      ncclResult_t enq = ncclSuccess;  // first failed enqueue; the group is still closed below
      for (size_t k = 0; k < parts.size() && enq == ncclSuccess; k++) {
        DevSession& d = *parts[k];
        HIPCHK(hipSetDevice(d.device));
        enq = ncclAllReduce(d.cn.p, d.cn.p, nrules * KV_HIST, ncclUint64, ncclSum, comms[k], d.stream);
        if (scopes && enq == ncclSuccess)
          enq = ncclAllReduce(d.scn.p, d.scn.p, (size_t)d.nscopes * nrules * KV_HIST, ncclUint64, ncclSum, comms[k],
                              d.stream);
      }
      const ncclResult_t end = ncclGroupEnd();
      if (enq != ncclSuccess) abort_comms(std::string("ncclAllReduce failed: ") + ncclGetErrorString(enq));
      if (end != ncclSuccess) abort_comms(std::string("RCCL all-reduce failed: ") + ncclGetErrorString(end));
      for (auto& d : parts) {
        HIPCHK(hipSetDevice(d->device));
        if (hipStreamSynchronize(d->stream) != hipSuccess) abort_comms("RCCL all-reduce: stream synchronize failed");
      }
      counts_ = parts[0]->read_counts();
      if (scopes) scope_counts_ = parts[0]->read_scope_counts();
    } else {
      for (auto& d : parts) {
        std::vector<int64_t> c = d->read_counts();
        for (size_t i = 0; i < c.size(); i++) counts_[i] += c[i];
        if (scopes) {
          std::vector<int64_t> sc = d->read_scope_counts();
          if (scope_counts_.empty()) scope_counts_.assign(sc.size(), 0);
          for (size_t i = 0; i < sc.size(); i++) scope_counts_[i] += sc[i];
        }
      }
    }
    reduced = true;
  }
  void fetch(kv_result* out, double ms) {
    if (parts_mode) throw std::runtime_error("kv_session_fetch: a parts session keeps no host batch");
    out->ps = &ps->ps;
    out->b = bt;
    out->n_rules = nrules;
    out->n_res = nres;
    out->mode = mode;
    out->kernel_ms = ms;
    reduce();
    out->counts = counts_;
    if (mode & KV_MODE_SCOPES) out->scope_counts = scope_counts_;
    out->sparse = parts[0]->O.status && parts[0]->O.sflag && (mode & (KV_MODE_STATUS | KV_MODE_ERRORS)) && nres &&
                  nrules && std::all_of(parts.begin(), parts.end(), [](const auto& p) { return p->rec_compact; });
    if (parts[0]->O.status && (mode & (KV_MODE_STATUS | KV_MODE_ERRORS)) && !out->sparse) {
      HIPCHK(hipSetDevice(parts[0]->device));
      const auto ta = std::chrono::steady_clock::now();
      out->status.alloc(nrules * nres);
      out->phases.push_back(
          {"host_alloc", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count()});
    }
    out->errors = (mode & KV_MODE_ERRORS) != 0;
    out->parts.resize(parts.size());
    for (size_t k = 0; k < parts.size(); k++) {
      out->parts[k].lo = ranges[k].first;
      out->parts[k].n = ranges[k].second - ranges[k].first;
      if (!shards.empty()) out->parts[k].shard = shards[k];
    }
    each([&](size_t k) { parts[k]->fetch(out, &out->parts[k], ranges[k].first, nres); });
  }
};

// devices of a mask, each repeated KVGPU_SHARDS_PER_DEVICE times (logical shards: the
// multi-device path on one GPU, for tests; counts are then summed on the host)
std::vector<int> mask_devices(uint32_t mask) {
  std::vector<int> d;
  int per = 1;
  if (const char* e = getenv("KVGPU_SHARDS_PER_DEVICE")) per = std::max(1, atoi(e));
  for (int i = 0; i < 32; i++)
    if (mask & (1u << i))
      for (int k = 0; k < per; k++) d.push_back(i);
  return d;
}

void run(kv_policyset* ps, kv_batch* bt, const char* ctx_json, const std::vector<int>& devices, uint32_t mode,
         kv_result* out, int warmup, int iters, double* ms) {
  if (devices.empty()) throw std::runtime_error("empty device mask");
  const auto t0 = std::chrono::steady_clock::now();
  SessionSet s(ps, bt, ctx_json, devices, mode);
  const auto t1 = std::chrono::steady_clock::now();
  if (warmup > 0) s.run(warmup);
  int n = std::max(iters, 1);
  double t = s.run(n) / n;
  const auto t2 = std::chrono::steady_clock::now();
  if (ms) *ms = t;
  if (out) {
    auto d = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const double up = s.parts.empty() ? 0.0 : s.parts[0]->upload_ms;
    out->phases = {{"upload", up}, {"setup", d(t0, t1) - up}, {"pass", d(t1, t2)}};
    // the precondition gate's kernel (HIP events; it ran when the batch was first uploaded)
    if (!ps->ps.csets.empty() && !s.parts.empty() && s.parts[0]->batch_ref)
      out->phases.push_back({"precond", s.parts[0]->batch_ref->pre_ms});
    // the deny fold's kernel, likewise
    if (!ps->ps.dsets.empty() && !s.parts.empty() && s.parts[0]->batch_ref)
      out->phases.push_back({"deny", s.parts[0]->batch_ref->deny_ms});
    // the foreach fold's two kernels, likewise
    if (!ps->ps.fsets.empty() && !s.parts.empty() && s.parts[0]->batch_ref)
      out->phases.push_back({"foreach", s.parts[0]->batch_ref->fe_ms});
    s.fetch(out, t);
  }
  if (getenv("KVGPU_VERBOSE")) {  // host-boundary breakdown
    const auto t3 = std::chrono::steady_clock::now();
    auto d = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "[kvgpu] kv_validate: setup+upload %.1f ms, passes %.1f ms, fetch %.1f ms\n", d(t0, t1), d(t1, t2),
            d(t2, t3));
  }
}

}  // namespace

struct kv_session {
  SessionSet set;
  kv_session(kv_policyset* p, kv_batch* b, const char* ctx_json, const std::vector<int>& devices, uint32_t m)
      : set(p, b, ctx_json, devices, m) {}
  kv_session(kv_policyset* p, const char* ctx_json, uint32_t m, uint32_t n) : set(p, ctx_json, m, n) {}
};

namespace {

// kv_validate / kv_validate_devices: one pass over the devices, fetched
int validate_on(const kv_policyset* ps, const kv_batch* b, const char* ctx_json, const std::vector<int>& devices,
                uint32_t mode, kv_result** out, kv_error** err) {
  if (!ps || !b || !out) return fail(err, KV_E_INVALID, "null argument");
  if (b->owner != ps) return fail(err, KV_E_INVALID, "batch was ingested for a different policy set");
  auto r = std::make_unique<kv_result>();
  run(const_cast<kv_policyset*>(ps), const_cast<kv_batch*>(b), ctx_json, devices, mode, r.get(), 0, 1, nullptr);
  *out = r.release();
  return 0;
}

// kv_session_create / kv_session_create_devices
int session_on(const kv_policyset* ps, const kv_batch* b, const char* ctx_json, const std::vector<int>& devices,
               uint32_t mode, kv_session** out, kv_error** err) {
  if (!ps || !b || !out) return fail(err, KV_E_INVALID, "null argument");
  if (b->owner != ps) return fail(err, KV_E_INVALID, "batch was ingested for a different policy set");
  if (devices.empty()) return fail(err, KV_E_INVALID, "empty device mask");
  *out = new kv_session(const_cast<kv_policyset*>(ps), const_cast<kv_batch*>(b), ctx_json, devices, mode);
  return 0;
}

}  // namespace

extern "C" {

int kv_compile(const char* policies_json, size_t len, uint32_t flags, kv_policyset** out, kv_error** err) {
  if (!policies_json || !out) return fail(err, KV_E_INVALID, "null argument");
  if ((flags & KV_COMPILE_FOREACH_PATTERN) && !(flags & KV_COMPILE_FOREACH))
    return fail(err, KV_E_INVALID, "KV_COMPILE_FOREACH_PATTERN needs KV_COMPILE_FOREACH");
  if ((flags & KV_COMPILE_FOREACH_ENTRIES) && !(flags & KV_COMPILE_FOREACH))
    return fail(err, KV_E_INVALID, "KV_COMPILE_FOREACH_ENTRIES needs KV_COMPILE_FOREACH");
  if ((flags & KV_COMPILE_FOREACH_ANYPATTERN) &&
      (flags & (KV_COMPILE_FOREACH | KV_COMPILE_FOREACH_PATTERN)) != (KV_COMPILE_FOREACH | KV_COMPILE_FOREACH_PATTERN))
    return fail(err, KV_E_INVALID, "KV_COMPILE_FOREACH_ANYPATTERN needs KV_COMPILE_FOREACH | KV_COMPILE_FOREACH_PATTERN");
  if ((flags & KV_COMPILE_FOREACH_PATVARS) &&
      (flags & (KV_COMPILE_FOREACH | KV_COMPILE_FOREACH_PATTERN)) != (KV_COMPILE_FOREACH | KV_COMPILE_FOREACH_PATTERN))
    return fail(err, KV_E_INVALID, "KV_COMPILE_FOREACH_PATVARS needs KV_COMPILE_FOREACH | KV_COMPILE_FOREACH_PATTERN");
  return guarded(KV_E_PARSE, err, [&]() -> int {
    auto s = std::make_unique<kv_policyset>();
    compile_policies(policies_json, len, &s->ps,
                     flags & (KV_COMPILE_DENY | KV_COMPILE_FOREACH | KV_COMPILE_FOREACH_PATTERN | KV_COMPILE_FOREACH_ENTRIES |
                              KV_COMPILE_FOREACH_ANYPATTERN | KV_COMPILE_FOREACH_PATVARS));
    if (flags & KV_COMPILE_SPECIALIZE) {
      s->jit = std::make_unique<JitImage>();
      jit_build(s->ps, s->jit.get());  // (kvjitbuild.cpp: generate, plan, compile, variants)
    }
    *out = s.release();
    return 0;
  });
}

int kv_policyset_info(const kv_policyset* ps, uint32_t* n_policies, uint32_t* n_rules) {
  if (!ps) return KV_E_INVALID;
  if (n_policies) *n_policies = (uint32_t)ps->ps.policy_names.size();
  if (n_rules) *n_rules = (uint32_t)ps->ps.rules.size();
  return 0;
}

int kv_policyset_jit_info(const kv_policyset* ps, uint32_t* n_kernels, double* gen_ms, double* compile_ms,
                          uint64_t* code_bytes) {
  if (!ps) return KV_E_INVALID;
  const JitImage* j = ps->jit.get();
  if (n_kernels) *n_kernels = j ? (uint32_t)j->chunks.size() : 0;
  if (gen_ms) *gen_ms = j ? j->gen_ms : 0;
  if (compile_ms) *compile_ms = j ? j->compile_ms : 0;
  if (code_bytes) *code_bytes = j ? kvh::code_bytes(*j) : 0;
  return 0;
}

int kv_policyset_jit_cols(const kv_policyset* ps, uint32_t* n_wide, uint32_t* n_narrow) {
  if (!ps) return KV_E_INVALID;
  uint32_t w = 0, n = 0;
  if (const JitImage* j = ps->jit.get())
    for (const ColDesc& c : j->cols) (c.fmt == KV_COLF_NARROW ? n : w)++;
  if (n_wide) *n_wide = w;
  if (n_narrow) *n_narrow = n;
  return 0;
}

int kv_rule_info_get(const kv_policyset* ps, uint32_t rule, kv_rule_info* out) {
  if (!ps || !out) return KV_E_INVALID;
  if (rule >= ps->ps.rules.size()) return KV_E_RANGE;
  const RuleHost& rh = ps->ps.rhost[rule];
  const RuleRec& rr = ps->ps.rules[rule];
  out->policy = rh.policy;
  out->policy_name = ps->ps.policy_names[rh.policy].c_str();
  out->name = rh.name.c_str();
  out->route = rr.route;
  out->route_reason = rh.route_reason.c_str();
  out->message = rh.message.c_str();
  out->any_pattern = rh.anypattern ? 1 : 0;
  out->const_status = rr.const_status;
  out->const_message = rh.const_message.c_str();
  out->foreach_set = rh.foreach_set;
  return 0;
}

int kv_ingest(const kv_policyset* ps, const char* resources_json, size_t len, const char* ns_labels_json, kv_batch** out,
              kv_error** err) {
  if (!ps || !resources_json || !out) return fail(err, KV_E_INVALID, "null argument");
  return guarded(KV_E_PARSE, err, [&]() -> int {
    auto b = std::make_unique<kv_batch>();
    b->owner = ps;
    ingest_resources(ps->ps, resources_json, len, ns_labels_json, &b->b);
    if (getenv("KVGPU_VERBOSE"))
      fprintf(stderr, "[kvgpu] ingest: %zu resources, %zu cells, %zu vals, %zu string bytes\n", b->b.res.size(),
              (size_t)b->b.cells_used, b->b.vals.size(), b->b.strs.size());
    *out = b.release();
    return 0;
  });
}

int kv_batch_info(const kv_batch* b, uint64_t* n_res, uint64_t* store_bytes) {
  if (!b) return KV_E_INVALID;
  if (n_res) *n_res = b->b.res.size();
  if (store_bytes) *store_bytes = b->b.bytes_referenced;
  return 0;
}

int kv_batch_transfer_bytes(const kv_batch* b, uint64_t* bytes) {
  if (!b || !bytes) return KV_E_INVALID;
  *bytes = b->b.transfer_bytes();
  return 0;
}

int kv_validate(const kv_policyset* ps, const kv_batch* b, const char* ctx_json, int device, uint32_t mode,
                kv_result** out, kv_error** err) {
  return guarded(KV_E_PARSE, err, [&]() -> int { return validate_on(ps, b, ctx_json, {device}, mode, out, err); });
}

int kv_validate_devices(const kv_policyset* ps, const kv_batch* b, const char* ctx_json, uint32_t device_mask,
                        uint32_t mode, kv_result** out, kv_error** err) {
  return guarded(KV_E_PARSE, err,
                 [&]() -> int { return validate_on(ps, b, ctx_json, mask_devices(device_mask), mode, out, err); });
}

int kv_bench(const kv_policyset* ps, const kv_batch* b, const char* ctx_json, int device, uint32_t mode, int warmup,
             int iters, double* ms_per_iter, kv_error** err) {
  if (!ps || !b || !ms_per_iter) return fail(err, KV_E_INVALID, "null argument");
  return guarded(KV_E_PARSE, err, [&]() -> int {
    run(const_cast<kv_policyset*>(ps), const_cast<kv_batch*>(b), ctx_json, {device}, mode, nullptr, warmup, iters,
        ms_per_iter);
    return 0;
  });
}

int kv_batch_namespaces(const kv_batch* b, uint32_t* n) {
  if (!b || !n) return KV_E_INVALID;
  *n = (uint32_t)b->b.namespaces.size();
  return 0;
}

const char* kv_batch_namespace(const kv_batch* b, uint32_t i) {
  if (!b || i >= b->b.namespaces.size()) return nullptr;
  return b->b.namespaces[i].c_str();
}

int kv_condition_eval(const char* condition_json, size_t len, int* result) {
  if (!condition_json || !result) return KV_E_INVALID;
  return guarded(KV_E_PARSE, nullptr, [&]() -> int {
    JDoc d;
    parse_json(condition_json, len, NUM_FLOAT, &d);
    if (d.at(d.root).t != J_MAP) return KV_E_PARSE;
    const int64_t kn = d.get(d.root, "key"), on = d.get(d.root, "operator"), vn = d.get(d.root, "value");
    std::string op;
    if (on >= 0) {
      if (d.at((uint32_t)on).t != J_STR) return KV_E_PARSE;  // (json: cannot unmarshal into ConditionOperator)
      op = std::string(d.sval(d.at((uint32_t)on)));
    }
    const PV key = kn >= 0 ? to_pv(d, (uint32_t)kn) : PV{}, value = vn >= 0 ? to_pv(d, (uint32_t)vn) : PV{};
    bool range = false;
    const bool v = cond_eval(cond_op(op), key, value, &range);
    if (range) return KV_E_RANGE;
    *result = v ? 1 : 0;
    return 0;
  });
}

int kv_session_create(const kv_policyset* ps, const kv_batch* b, const char* ctx_json, int device, uint32_t mode,
                      kv_session** out, kv_error** err) {
  return guarded(KV_E_PARSE, err, [&]() -> int { return session_on(ps, b, ctx_json, {device}, mode, out, err); });
}

int kv_session_create_devices(const kv_policyset* ps, const kv_batch* b, const char* ctx_json, uint32_t device_mask,
                              uint32_t mode, kv_session** out, kv_error** err) {
  return guarded(KV_E_PARSE, err,
                 [&]() -> int { return session_on(ps, b, ctx_json, mask_devices(device_mask), mode, out, err); });
}

int kv_session_create_parts(const kv_policyset* ps, const char* ctx_json, uint32_t mode, uint32_t n_parts,
                            kv_session** out, kv_error** err) {
  if (!ps || !out || n_parts == 0) return fail(err, KV_E_INVALID, "bad argument");
  return guarded(KV_E_PARSE, err, [&]() -> int {
    *out = new kv_session(const_cast<kv_policyset*>(ps), ctx_json, mode, n_parts);
    return 0;
  });
}

int kv_session_attach_part(kv_session* s, uint32_t part, const kv_batch* b, int device, kv_error** err) {
  if (!s || !b) return fail(err, KV_E_INVALID, "null argument");
  if (b->owner != s->set.ps) return fail(err, KV_E_INVALID, "batch was ingested for a different policy set");
  return guarded(KV_E_INVALID, err, [&]() -> int {
    s->set.attach(part, const_cast<kv_batch*>(b), device);
    return 0;
  });
}

int kv_session_scopes(const kv_session* s, uint32_t* n_scopes) {
  if (!s || !n_scopes) return KV_E_INVALID;
  if (s->set.parts_mode) {
    if (!s->set.finalized) return KV_E_INVALID;
    *n_scopes = (uint32_t)s->set.scope_names.size();
  } else {
    *n_scopes = (uint32_t)s->set.bt->b.namespaces.size();
  }
  return 0;
}

const char* kv_session_scope_name(const kv_session* s, uint32_t i) {
  if (!s) return nullptr;
  const std::vector<std::string>& v = s->set.parts_mode ? s->set.scope_names : s->set.bt->b.namespaces;
  return i < v.size() ? v[i].c_str() : nullptr;
}

int kv_session_rccl_ranks(const kv_session* s, int* ranks) {
  if (!s || !ranks) return KV_E_INVALID;
  *ranks = s->set.rccl_ranks();
  return *ranks < 0 ? KV_E_DEVICE : 0;
}

int kv_session_status_bytes(kv_session* s, uint64_t* bytes) {
  if (!s || !bytes) return KV_E_INVALID;
  return guarded(KV_E_DEVICE, nullptr, [&]() -> int {
    uint64_t t = 0;
    for (auto& p : s->set.parts)
      if (p) t += p->written_status_bytes();
    *bytes = t;
    return 0;
  });
}

int kv_session_part_ms(const kv_session* s, double* ms) {
  if (!s || !ms) return KV_E_INVALID;
  for (size_t k = 0; k < s->set.parts.size(); k++) ms[k] = k < s->set.part_ms.size() ? s->set.part_ms[k] : 0.0;
  return 0;
}

int kv_session_parts(const kv_session* s, uint32_t* n_parts) {
  if (!s || !n_parts) return KV_E_INVALID;
  *n_parts = (uint32_t)s->set.parts.size();
  return 0;
}

int kv_session_fetch(kv_session* s, kv_result** out, kv_error** err) {
  if (!s || !out) return fail(err, KV_E_INVALID, "null argument");
  return guarded(KV_E_DEVICE, err, [&]() -> int {
    auto r = std::make_unique<kv_result>();
    s->set.fetch(r.get(), 0.0);
    *out = r.release();
    return 0;
  });
}

int kv_session_run(kv_session* s, int iters, double* event_ms, kv_error** err) {
  if (!s || iters < 0) return fail(err, KV_E_INVALID, "bad argument");
  return guarded(KV_E_DEVICE, err, [&]() -> int {
    double t = s->set.run(iters);
    if (event_ms) *event_ms = t;
    return 0;
  });
}

int kv_session_counts(kv_session* s, int64_t* counts) {
  if (!s || !counts) return KV_E_INVALID;
  return guarded(KV_E_DEVICE, nullptr, [&]() -> int {
    s->set.reduce();
    std::copy(s->set.counts_.begin(), s->set.counts_.end(), counts);
    return 0;
  });
}

int kv_session_scope_counts(kv_session* s, int64_t* counts) {
  if (!s || !counts || !(s->set.mode & KV_MODE_SCOPES)) return KV_E_INVALID;
  return guarded(KV_E_DEVICE, nullptr, [&]() -> int {
    s->set.reduce();
    std::copy(s->set.scope_counts_.begin(), s->set.scope_counts_.end(), counts);
    return 0;
  });
}

void kv_free_session(kv_session* s) { delete s; }

void kv_free_policyset(kv_policyset* ps) { delete ps; }
void kv_free_batch(kv_batch* b) { delete b; }
void kv_free_result(kv_result* r) { delete r; }
void kv_free_error(kv_error* e) {
  if (e) {
    free(e->message);
    free(e);
  }
}
void kv_free_buffer(char* p) { free(p); }

}  // extern "C"
