// Specialized kernels for a compiled policy set (see kvjit.hpp): the source generator. String emission
// over a PolicySet: no HIP, no hiprtc, no process, no file (kvjitbuild.cpp compiles the programs).
//
// Every GPU-routed rule's bytecode program (kvcompile.cpp) is re-emitted as a
// device function whose statements are the interpreter's op semantics
// (kvkernel.hip) with the operands folded in: key slots, predicate constants,
// glob segment words and quantity operands become immediates, the cursor stack
// becomes registers c0..cN, and the interpreter's parked-lane wake-up pcs
// (skip / catch targets) become gotos that each lane takes on its own (the
// hardware exec mask runs the divergence). Rule functions are inlined into
// chunk kernels, so lookups shared by several rules (root -> spec ->
// containers ...) are loaded once per chunk (the node store is __restrict__).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>
#include <unordered_map>

#include "kvjit.hpp"
#include "kvdevtypes.h"

namespace kvh {

using namespace kv;

namespace {

const char* kPrelude =
#include "kvjit_prelude.inc"
    ;

std::string hex32(uint32_t v) {
  char b[16];
  snprintf(b, sizeof b, "0x%08xu", v);
  return b;
}
// rules whose status is final after match / route: the other routes, and device deny rules
// (RuleRec::deny: their status is a byte of DevBatch::deny_st, they have no pattern program)
bool no_program(const RuleRec& rr) { return rr.route != 0 || rr.deny != 0; }
std::string u32(uint32_t v) { return std::to_string(v) + "u"; }
std::string u64(uint64_t v) { return std::to_string(v) + "ull"; }
std::string i64(int64_t v) {
  if (v == INT64_MIN) return "(-9223372036854775807ll - 1)";
  return std::to_string(v) + "ll";
}
std::string f64(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return "__longlong_as_double(" + i64((int64_t)b) + ")";
}

// rule groups of at least this many members write their records at the resource's slot of the
// record row; the other rules append theirs to the wave's segment (kvdevfn.h kv_gfin). Round 4
// (gpurun_out/ab3, ms per pass / GB written): from 16 members C2 0.720 / 0.47 (its 20- and
// 21-member image-glob groups go to slots), C3 8.22 / 9.7; from 22 C2 0.701 / 0.40, C3 8.24 /
// 9.4; never C2 0.699 / 0.40, C3 9.13 / 7.5.
constexpr uint32_t kGslotMembers = 22u;

// The generator's tuning environment, read once per jit_generate. Every one of these is part of
// the program text and so of the cache keys (code objects and plan):
//   KVGPU_JIT_NARROW=0   every path column wide (A/B runs; col_plan)
//   KVGPU_JIT_COLLOOPS=0 per-rule and nested array loops walk the node rows (A/B runs; emit_region)
//   KVGPU_JIT_STAMPS     the rule kernels stamp their segment boundaries (group_kernel, kJitStamps)
//   KVGPU_JIT_WAVES      first launch bound in waves per SIMD (default: at most 8, 0: none)
//   KVGPU_JIT_BLOCK_W    weight budget of the first block sizes (initial_blocks; default 160 / 240)
//   KVGPU_JIT_DIAG=A,B   diagnostics-only kernels (#define KV_DIAG_A ... ahead of the prelude; wrong results)
struct GenOpts {
  bool narrow, colloops, stamps, has_waves;
  int waves;
  uint32_t block_w;  // 0: the defaults
  std::string diag;  // the #define lines
  GenOpts() {
    const char* e = getenv("KVGPU_JIT_NARROW");
    narrow = !(e && e[0] == '0');
    e = getenv("KVGPU_JIT_COLLOOPS");
    colloops = !(e && e[0] == '0');
    stamps = getenv("KVGPU_JIT_STAMPS") != nullptr;
    e = getenv("KVGPU_JIT_WAVES");
    has_waves = e != nullptr;
    waves = e ? atoi(e) : 0;
    e = getenv("KVGPU_JIT_BLOCK_W");
    block_w = e && atoi(e) > 0 ? (uint32_t)atoi(e) : 0u;
    std::istringstream names((e = getenv("KVGPU_JIT_DIAG")) ? e : "");
    for (std::string t; std::getline(names, t, ',');)
      if (!t.empty()) diag += "#define KV_DIAG_" + t + " 1\n";
  }
};

struct Gen {
  struct Fam {
    std::string arr;                          // family array expr (family 0: ""; nested: "<parent's>[]<relative>")
    uint32_t parent = 0, arr_j = 0;           // the family and column that hold its array
    std::map<std::string, uint32_t> idx;      // relative expr -> column
    std::vector<std::vector<uint32_t>> steps; // per column: its path steps
    std::vector<uint32_t> use;                // per column: what the kernels read of it (ColUse)
  };
  // Structural form of a rule's program (group_form): rules of one form whose pattern nodes
  // differ by one constant can run as a rule group
  struct Form {
    std::string text;                      // empty: the rule cannot join a group
    std::vector<uint32_t> preds, pns;      // its leaf predicates and pattern nodes, in program order
    std::vector<uint32_t> leafpcs;         // its LEAF pcs relative to the program start
  };

  const PolicySet& ps;
  const GenOpts opt;

  // ================================================================ state of the image
  // Everything below lives for one jit_generate: ids are handed out in order of first use over
  // the whole image, and every one of them is part of the program text.
  //
  // value-predicate memo: a leaf predicate on a scalar is a pure function of the
  // (deduplicated) Val it reads, so each one is evaluated once per distinct value
  // of the batch (kvj_ptab) and the rule kernels test one bit of the table
  std::vector<uint32_t> mpreds;        // memo slot -> pred
  std::map<uint32_t, uint32_t> pslot;  // pred -> memo slot
  std::map<uint32_t, uint32_t> pmask;  // pred -> position classes of its leaves (leaf_classes)
  // path columns (below): the families, and the uses known before generation (JitImage::col_use)
  std::vector<Fam> fams;
  std::map<std::string, uint32_t> fam_of;  // family array expr -> family
  std::map<std::string, uint32_t> use_seed;
  // Site records of rule groups (kvdevtypes.h GSiteDesc): per group of 2+ members its descriptor
  // (n, gpre, moff, 0) in gs_desc and its members' (rule, pattern-node shift) in gs_mem, numbered
  // in generation order over the image (round 5, with the unwritten NOMATCH segments: C3 writes
  // 9.4 -> 2.9 GB per pass).
  std::vector<uint32_t> gs_desc, gs_mem;
  uint32_t gs_members = 0;
  // Match bits (kv_mtup_kernel): mt_bits[p] = the rule at bit position p (KV_SENT: padding), in
  // kernel and LDS-row order; a kernel's rows start at a word boundary (Kern::mt_kbase)
  std::vector<uint32_t> mt_bits;
  std::vector<uint8_t> rec_slot;  // rules whose records go to their resource slot (kGslotMembers)
  uint32_t gtab_n = 0;            // member tables emitted so far
  std::map<uint32_t, Form> forms;  // group_form of the rules asked for so far (form_of)
  // kvj_ptab register-path globs (qglob_fn)
  std::map<uint32_t, uint32_t> bslot;                 // byte -> slot of bm[]
  std::map<uint32_t, std::set<uint32_t>> glob_bytes;  // atom -> bytes its middle segments search
  // helper functions (name, text) in generation order, which is dependency order: a helper's
  // callees are emitted before its own text. Each is emitted once (the done-sets).
  std::vector<std::pair<std::string, std::string>> helpers;
  std::set<uint32_t> globs_done, atoms_done, preds_done, blks_done;
  std::set<std::pair<char, uint32_t>> qglobs_done, qatoms_done, qpreds_done;
  bool dleaf_done = false;
  // kernel texts (name, source): each one is compiled as its own hiprtc program after the
  // helpers it reaches (jit_generate)
  std::vector<std::pair<std::string, std::string>> kernels;

  // ================================================================ state of one kernel
  // The rule kernel being generated: group_kernel owns it and hands it to its blocks (a block's
  // own state is struct Block, below)
  struct Kern {
    uint32_t mt_kbase = 0;      // first match word of the kernel: LDS row q has bit 32 * mt_kbase + q
    uint32_t gs0 = 0, gsn = 0;  // site-record groups: the kernel's first (of the image) and its count
    std::string decls;          // declarations its blocks need ahead of the kernel (member tables)
    bool grouped = false;       // hoist regions in three parts (JitKernelPlan::grouped)
    bool colloops = false;      // per-rule array loops over path columns (JitKernelPlan::colloops)
  };

  explicit Gen(const PolicySet& p) : ps(p), rec_slot(p.rules.size(), 0) {
    fams.emplace_back();
    col_of(0, "R");  // column 0 of family 0: the root
  }

  // a helper function's text, recorded under its name when it is complete
  struct Helper : std::ostringstream {
    Gen& g;
    const std::string name;
    Helper(Gen& gg, std::string n) : g(gg), name(std::move(n)) {}
    ~Helper() { g.helpers.push_back({name, str()}); }
  };
  static std::string num(const char* prefix, uint32_t i) { return prefix + std::to_string(i); }

  // ---------------------------------------------------------------- path columns
  // Hoisted lookups (below) read the node at their static path from a column of the batch
  // (kvdevtypes.h, built per batch by kvcol.h) instead of walking the node rows from the root
  // or the loop element: one independent coalesced load per lookup instead of a chain of
  // dependent ones. Family 0 holds root paths; family f > 0 the paths relative to the elements
  // of one array path (a column of family 0), or of one array path relative to the elements of
  // such a family (a nested family: kvdevtypes.h). Columns are numbered in order of first use; the
  // kernels read column j of family f through macros (KVC_LD_<f>_<j> and its kin, col_plan)
  // defined at the head of every kernel program once the whole image is generated and the
  // cell format of every column is known.
  // Cell format of a column (kvdevtypes.h ColFmt): narrow unless a consumer, marked where it is
  // emitted, reads more of a cell than its presence, its type and a scalar's Val id. CU_WIDE: a
  // field of the node (.a / .b / .c) or a map's own node index is read; CU_B: the node's b is
  // (an array's element count); CU_LEAF: a leaf predicate reads it (its array case needs a and b
  // when the cell is wide, and reads the array's node when it is narrow: kv_leaf_fix). The uses of every
  // rule of the policy set decide, whatever the kernel plan; KVGPU_JIT_NARROW=0 makes every
  // column wide (GenOpts).
  enum ColUse : uint32_t { CU_WIDE = 1u, CU_B = 2u, CU_LEAF = 4u };
  void col_mark(int fam, uint32_t j, uint32_t use) {
    if (fam >= 0 && j != kNoCol) fams.at((size_t)fam).use.at(j) |= use;
  }
  static std::string col_macro(const char* what, uint32_t f, uint32_t j) {
    return std::string("KVC_") + what + "_" + std::to_string(f) + "_" + std::to_string(j);
  }
  static constexpr uint32_t kNoCol = 0xFFFFFFFFu;
  // steps of a symbolic path: "/s<slot>" (slot-addressed map) or "/k<key>" (keep-all map
  // scan) after the root token ("R", or "E<tag>" of a loop element, or nothing)
  static bool expr_steps(const std::string& ex, std::vector<uint32_t>* out) {
    out->clear();
    size_t at = ex.find('/');
    while (at != std::string::npos) {
      const size_t nx = ex.find('/', at + 1);
      const std::string tok = ex.substr(at + 1, nx == std::string::npos ? std::string::npos : nx - at - 1);
      if (tok.size() < 2 || (tok[0] != 's' && tok[0] != 'k')) return false;
      const unsigned long v = strtoul(tok.c_str() + 1, nullptr, 10);
      if (v >= KV_COL_SCAN) return false;
      out->push_back((uint32_t)v | (tok[0] == 'k' ? KV_COL_SCAN : 0u));
      at = nx;
    }
    return out->size() <= KV_COL_MAXD;
  }
  uint32_t col_of(uint32_t f, const std::string& rel) {
    Fam& F = fams.at(f);
    auto it = F.idx.find(rel);
    if (it != F.idx.end()) return it->second;
    std::vector<uint32_t> st;
    if (!expr_steps(rel, &st)) return kNoCol;
    const uint32_t j = (uint32_t)F.steps.size();
    F.idx.emplace(rel, j);
    F.steps.push_back(st);
    F.use.push_back(0u);
    return j;
  }
  // family of the elements of the array at `rel` in family `parent` (0: a root path; f > 0: a
  // path relative to the elements of f, itself a family of a root path: two levels only); its
  // column 0 is the element itself
  uint32_t family(uint32_t parent, const std::string& rel) {
    if (parent && fams.at(parent).parent) return kNoCol;
    const std::string arr = parent ? fams[parent].arr + "[]" + rel : rel;
    auto it = fam_of.find(arr);
    if (it != fam_of.end()) return it->second;
    const uint32_t j = col_of(parent, rel);
    if (j == kNoCol) return kNoCol;
    const uint32_t f = (uint32_t)fams.size();
    fams.emplace_back();
    fams.back().arr = arr;
    fams.back().parent = parent;
    fams.back().arr_j = j;
    col_of(f, "");
    fam_of.emplace(arr, f);
    return f;
  }
  uint32_t family(const std::string& arr) { return family(0, arr); }
  // the plan (JitImage::cols / fam_*) and the macro block of the kernel programs: per family
  // the words of a row (KVC_W<f>), per column its load from the row at word `b` (KVC_LD), the
  // node index of a map cell (KVC_IX) and the table word of a leaf on it: whole, array case
  // inline (KVC_LO, regions in first-use order), or as the gather (KVC_LW) and the word of an
  // array cell (KVC_LA, the fix-up) of a region in three parts
  void col_plan(JitImage* out, std::string* defs) const {
    out->cols.clear();
    out->fam_arr.clear();
    out->fam_parent.clear();
    out->fam_ncols.clear();
    out->fam_nw.clear();
    out->fam_nb.clear();
    out->fam_nn.clear();
    out->col_use.clear();
    std::ostringstream d;
    // (a hoisted leaf on a node read from the node rows: the whole node is there)
    d << "#define KVC_LO_ROW(n, w) kv_leaf_word(P, N, n, w)\n"
      << "#define KVC_LW_ROW(n, w) kv_leaf_gather(P, n, w)\n"
      << "#define KVC_LA_ROW(n, w) kv_leaf_fix(P.ptab, P.n_vals, N, (n).a, (n).b, false, w)\n";
    std::vector<uint32_t> col0(fams.size(), 0u);  // first column of each family in out->cols
    for (uint32_t f = 1; f < fams.size(); f++) col0[f] = col0[f - 1] + (uint32_t)fams[f - 1].steps.size();
    std::set<std::pair<uint32_t, uint32_t>> arrs;  // the family arrays: (family, column)
    for (uint32_t f = 1; f < fams.size(); f++) arrs.insert({fams[f].parent, fams[f].arr_j});
    for (uint32_t f = 0; f < fams.size(); f++) {
      const Fam& F = fams[f];
      out->fam_arr.push_back(f ? col0[F.parent] + F.arr_j : 0u);
      out->fam_parent.push_back(F.parent);
      out->fam_ncols.push_back((uint32_t)F.steps.size());
      std::vector<uint32_t> use(F.steps.size(), 0u);
      for (const auto& kv : F.idx) {
        const std::string key = F.arr + "|" + kv.first;
        uint32_t u = F.use[kv.second];
        auto it = use_seed.find(key);
        if (it != use_seed.end()) u |= it->second;
        if (arrs.count({f, kv.second})) u |= CU_WIDE | CU_B;  // a family array: a, b, c
        use[kv.second] = u;
        out->col_use[key] = u;
      }
      uint32_t nw = 0, nb = 0, nn = 0;
      const size_t c0 = out->cols.size();
      for (uint32_t j = 0; j < F.steps.size(); j++) {
        ColDesc c{};
        c.fam = f;
        c.j = j;
        c.nsteps = (uint32_t)F.steps[j].size();
        for (uint32_t s = 0; s < c.nsteps; s++) c.steps[s] = F.steps[j][s];
        if (opt.narrow && !(use[j] & CU_WIDE)) {
          c.fmt = KV_COLF_NARROW;
          c.pos = nn++;
        } else {
          c.pos = nw++;
          c.fmt = KV_COLF_WIDE;
          if (use[j] & (CU_B | CU_LEAF)) {
            c.fmt = KV_COLF_WIDEB;
            c.bpos = nb++;
          }
        }
        out->cols.push_back(c);
      }
      out->fam_nw.push_back(nw);
      out->fam_nb.push_back(nb);
      out->fam_nn.push_back(nn);
      d << "#define KVC_W" << f << " " << (3u * nw + nb + nn) * KV_LANES << "u\n";
      for (uint32_t j = 0; j < F.steps.size(); j++) {
        const ColDesc& c = out->cols[c0 + j];
        d << "#define " << col_macro("LD", f, j) << "(b) ";
        if (c.fmt == KV_COLF_NARROW) {
          d << "kv_ldn(PC, (b) + " << u32((3u * nw + nb + c.pos) * KV_LANES) << " + ln_)\n"
            << "#define " << col_macro("IX", f, j) << "(n) (node_type((n).kt) == NT_MAP ? KV_NARROW_IDX : 0u)\n"
            << "#define " << col_macro("LO", f, j) << "(n, w) kv_leaf_word_n(P, N, n, w)\n"
            << "#define " << col_macro("LW", f, j) << "(n, w) kv_leaf_gather(P, n, w)\n"
            << "#define " << col_macro("LA", f, j) << "(n, w) kv_leaf_fix(P.ptab, P.n_vals, N, (n).a, 0u, true, w)\n";
        } else {
          if (c.fmt == KV_COLF_WIDEB)
            d << "kv_ldwb(PC, (b) + " << u32(c.pos * 3u * KV_LANES) << " + 3u * ln_, (b) + "
              << u32((3u * nw + c.bpos) * KV_LANES) << " + ln_)\n";
          else
            d << "kv_ldw(PC, (b) + " << u32(c.pos * 3u * KV_LANES) << " + 3u * ln_)\n";
          d << "#define " << col_macro("IX", f, j) << "(n) (node_type((n).kt) == NT_MAP ? (n).c : 0u)\n"
            << "#define " << col_macro("LO", f, j) << "(n, w) kv_leaf_word(P, N, n, w)\n"
            << "#define " << col_macro("LW", f, j) << "(n, w) kv_leaf_gather(P, n, w)\n"
            << "#define " << col_macro("LA", f, j) << "(n, w) kv_leaf_fix(P.ptab, P.n_vals, N, (n).a, (n).b, false, w)\n";
        }
      }
    }
    for (uint32_t f = 1; f < fams.size(); f++) out->cols.at(out->fam_arr[f]).arr_fam = f;
    *defs = d.str();
  }

  // every atom of string predicate pi (none of another kind), in alternative and conjunct order
  template <class Fn>
  void each_atom(uint32_t pi, Fn fn) const {
    const Pred& pr = ps.preds[pi];
    if (pr.kind != PK_STRING) return;
    for (uint32_t a = pr.first; a < pr.first + pr.count; a++)
      for (uint32_t c = ps.alts[a].first; c < ps.alts[a].first + ps.alts[a].count; c++) {
        fn(ps.conjs[c].a0);
        if (ps.conjs[c].kind != CJ_ATOM) fn(ps.conjs[c].a1);
      }
  }

  // ---------------------------------------------------------------- globs
  // word compare of segment `sg` against value bytes [k, k + len) (base 4-byte aligned)
  std::string seg_expr(const GSeg& sg, const std::string& k, bool aligned0) {
    const uint32_t nw = (sg.len + 3) / 4;
    std::ostringstream e;
    e << "([&]() -> bool { ";
    if (aligned0) {
      e << "uint32_t x = 0u; ";
      for (uint32_t i = 0; i < nw; i++) {
        const GWord& g = ps.gwords[sg.wfirst + i];
        if (g.mask == 0) continue;
        e << "x |= (base[" << i << "] ^ " << hex32(g.w) << ") & " << hex32(g.mask) << "; ";
      }
      e << "return x == 0u; })()";
      return e.str();
    }
    e << "const uint32_t k_ = " << k << ", a_ = k_ >> 2, sh_ = k_ & 3u; uint32_t lo_ = base[a_], hi_, x = 0u; ";
    for (uint32_t i = 0; i < nw; i++) {
      const GWord& g = ps.gwords[sg.wfirst + i];
      e << "hi_ = base[a_ + " << (i + 1) << "]; ";
      if (g.mask) e << "x |= (__builtin_amdgcn_alignbyte(hi_, lo_, sh_) ^ " << hex32(g.w) << ") & " << hex32(g.mask) << "; ";
      e << "lo_ = hi_; ";
    }
    e << "return x == 0u; })()";
    return e.str();
  }

  void glob_fn(uint32_t ai) {
    if (!globs_done.insert(ai).second) return;
    const Atom& A = ps.atoms[ai];
    Helper o(*this, num("g_glob_", ai));
    o << "__device__ __forceinline__ bool " << o.name
      << "(const uint8_t* __restrict__ s, uint32_t sl, bool ascii, const uint8_t* __restrict__ pstr) {\n";
    const uint32_t fl = A.gflags;
    if (fl & G_ALL) { o << "  return true;\n}\n"; return; }
    if (fl & G_EMPTY) { o << "  return sl == 0u;\n}\n"; return; }
    if (fl & G_HASQ)
      o << "  if (!ascii) return kv_glob(pstr + " << u32(A.s_off) << ", " << u32(A.s_len & 0x7FFFFFFFu) << ", s, sl);\n";
    o << "  if (sl < " << u32(A.gmin) << ") return false;\n";
    o << "  const uint32_t* __restrict__ base = (const uint32_t*)s;\n";
    const uint32_t n = A.gcount;
    const GSeg* segs = ps.gsegs.data() + A.gfirst;
    uint32_t i0 = 0, i1 = n;
    o << "  uint32_t pos = 0u, end = sl;\n";
    if (!(fl & G_LEAD)) {
      const GSeg& s0 = segs[0];
      if (n == 1 && !(fl & G_TRAIL)) {
        o << "  return sl == " << u32(s0.len) << " && " << seg_expr(s0, "0u", true) << ";\n}\n";
        return;
      }
      o << "  if (!" << seg_expr(s0, "0u", true) << ") return false;\n";
      o << "  pos = " << u32(s0.len) << ";\n";
      i0 = 1;
    }
    if (!(fl & G_TRAIL)) {
      const GSeg& st = segs[n - 1];
      o << "  if (end < pos + " << u32(st.len) << ") return false;\n";
      o << "  if (!" << seg_expr(st, "end - " + u32(st.len), false) << ") return false;\n";
      o << "  end -= " << u32(st.len) << ";\n";
      i1 = n - 1;
    }
    for (uint32_t i = i0; i < i1; i++) {
      const GSeg& sg = segs[i];
      // leftmost occurrence of the segment in [pos, end): candidates are the
      // positions of its first literal byte, found 4 bytes at a time (SWAR
      // zero-byte test, exact: it never misses a match, false candidates are
      // rejected by the full word compare)
      const auto [j, cbyte] = seg_key(sg);
      if (j < 0) {  // all-'?' segment: plain scan
        o << "  { bool found = false;\n"
          << "    for (uint32_t k = pos; k + " << u32(sg.len) << " <= end; k++)\n"
          << "      if (" << seg_expr(sg, "k", false) << ") { pos = k + " << u32(sg.len) << "; found = true; break; }\n"
          << "    if (!found) return false; }\n";
        continue;
      }
      o << "  { if (end < pos + " << u32(sg.len) << ") return false;\n"
        << "    const uint32_t plo = pos + " << u32(j) << ", phi = end - " << u32(sg.len) << " + " << u32(j) << ";\n"
        << "    bool found = false;\n"
        << "    for (uint32_t wa = plo >> 2; wa <= (phi >> 2) && !found; wa++) {\n"
        << "      const uint32_t w = base[wa] ^ " << hex32(cbyte * 0x01010101u) << ";\n"
        << "      uint32_t m = (w - 0x01010101u) & ~w & 0x80808080u;\n"
        << "      while (m) {\n"
        << "        const uint32_t p = wa * 4u + ((uint32_t)__builtin_ctz(m) >> 3); m &= m - 1u;\n"
        << "        if (p < plo || p > phi) continue;\n"
        << "        const uint32_t k = p - " << u32(j) << ";\n"
        << "        if (" << seg_expr(sg, "k", false) << ") { pos = k + " << u32(sg.len) << "; found = true; break; }\n"
        << "      }\n"
        << "    }\n"
        << "    if (!found) return false; }\n";
    }
    o << "  (void)pos; (void)end;\n  return true;\n}\n";
  }

  // ---------------------------------------------------------------- kvj_ptab globs (register path)
  // In kvj_ptab a value's bytes (<= 64) sit in 16 registers `w` (plus an LDS copy
  // `lw` for reads at a per-lane offset). A middle segment's candidates are the
  // positions of one of its literal bytes, taken from a 64-bit byte mask `bm[slot]`
  // that the row computes once per distinct byte (kv_bmask: straight-line SWAR over
  // the 16 words) and that every glob of the row sharing that byte reuses; the
  // leftmost verified candidate at or after `pos` wins (the same leftmost-occurrence
  // search as glob_fn, without the per-lane word loop that made the kernel
  // scalar-issue bound: 2.1e8 SALU against 6.0e7 VALU instructions per pass on C2).
  static constexpr uint32_t kMaxBSlots = 48;
  // register-path variants: values of <= 64 bytes (16 words, 64-bit masks, prefix q_) and
  // of <= 128 bytes (32 words, two-word masks KvM2, prefix r_); the mask helpers
  // (kv_mrange / kv_mctz / kv_mpop) are overloaded on the mask type
  struct QV {
    char pfx;
    const char* mt;   // mask type
    const char* bmk;  // mask builder
    uint32_t words;
  };
  static constexpr QV kQ64{'q', "uint64_t", "kv_bmask", 16}, kQ128{'r', "KvM2", "kv_bmask2", 32};

  // first literal byte of segment `sg` and its offset in the segment (-1: all '?')
  std::pair<int32_t, uint32_t> seg_key(const GSeg& sg) const {
    for (uint32_t q = 0; q < sg.len; q++) {
      const GWord& gw = ps.gwords[sg.wfirst + q / 4];
      if ((gw.mask >> (8 * (q % 4))) & 0xFFu) return {(int32_t)q, (gw.w >> (8 * (q % 4))) & 0xFFu};
    }
    return {-1, 0u};
  }

  std::string qsig(const QV& v) const {
    return std::string("(const Val* __restrict__ V, const uint8_t* __restrict__ S, const uint32_t* w, const uint32_t* lw, const ") +
           v.mt + "* bm, const uint8_t* __restrict__ pstr, uint32_t type, const Node& n)";
  }

  void qglob_fn(uint32_t ai, const QV& v) {
    if (!qglobs_done.insert({v.pfx, ai}).second) return;
    const Atom& A = ps.atoms[ai];
    Helper q(*this, v.pfx + num("_glob_", ai));
    // branch-free: every step folds into `ok` (indices clamped so a failed step reads in
    // bounds); only a segment whose leftmost candidate fails verification loops over the rest
    q << "__device__ __forceinline__ bool " << q.name
      << "(const uint32_t* w, const uint32_t* lw, const " << v.mt << "* bm, uint32_t sl, bool ascii, "
         "const uint8_t* __restrict__ pstr) {\n";
    const uint32_t fl = A.gflags;
    if (fl & G_ALL) { q << "  return true;\n}\n"; return; }
    if (fl & G_EMPTY) { q << "  return sl == 0u;\n}\n"; return; }
    if (fl & G_HASQ)
      q << "  if (!ascii) return kv_glob(pstr + " << u32(A.s_off) << ", " << u32(A.s_len & 0x7FFFFFFFu)
        << ", (const uint8_t*)lw, sl);\n";
    const uint32_t n = A.gcount;
    const GSeg* segs = ps.gsegs.data() + A.gfirst;
    uint32_t i0 = 0, i1 = n;
    q << "  const uint32_t* base = lw;\n  bool ok = sl >= " << u32(A.gmin) << ";\n  uint32_t pos = 0u, end = sl;\n";
    auto prefix_expr = [&](const GSeg& sg) {  // aligned compare at 0 from the registers
      std::ostringstream e;
      e << "((0u";
      for (uint32_t i = 0; i < (sg.len + 3) / 4; i++) {
        const GWord& g = ps.gwords[sg.wfirst + i];
        if (g.mask) e << " | ((w[" << i << "] ^ " << hex32(g.w) << ") & " << hex32(g.mask) << ")";
      }
      e << ") == 0u)";
      return e.str();
    };
    if (!(fl & G_LEAD)) {
      const GSeg& s0 = segs[0];
      if (n == 1 && !(fl & G_TRAIL)) {
        q << "  return (sl == " << u32(s0.len) << ") & " << prefix_expr(s0) << ";\n}\n";
        return;
      }
      q << "  ok &= " << prefix_expr(s0) << ";\n  pos = " << u32(s0.len) << ";\n";
      i0 = 1;
    }
    if (!(fl & G_TRAIL)) {
      const GSeg& st = segs[n - 1];
      q << "  { const bool fit_ = ok & (end >= pos + " << u32(st.len) << ");\n"
        << "    const uint32_t ks_ = fit_ ? end - " << u32(st.len) << " : 0u;\n"
        << "    ok = fit_ & " << seg_expr(st, "ks_", false) << ";\n"
        << "    end = ks_; }\n";
      i1 = n - 1;
    }
    for (uint32_t i = i0; i < i1; i++) {
      const GSeg& sg = segs[i];
      const auto [j, cb] = seg_key(sg);
      if (j < 0) {  // all-'?' segment: its leftmost occurrence is pos itself
        q << "  ok &= end >= pos + " << u32(sg.len) << ";\n  pos += " << u32(sg.len) << ";\n";
        continue;
      }
      auto it = bslot.find(cb);
      if (it == bslot.end() && bslot.size() < kMaxBSlots) it = bslot.emplace(cb, (uint32_t)bslot.size()).first;
      const std::string mask =
          it != bslot.end() ? "bm[" + u32(it->second) + "]" : std::string(v.bmk) + "(w, " + hex32(cb * 0x01010101u) + ")";
      if (it != bslot.end()) glob_bytes[ai].insert(cb);
      // candidates p in [plo, phi] (phi < 4 * words: end <= sl and j < len)
      q << "  { ok &= end >= pos + " << u32(sg.len) << ";\n"
        << "    const uint32_t plo = ok ? pos + " << u32(j) << " : 0u, phi = ok ? end - " << u32(sg.len) << " + " << u32(j)
        << " : 0u;\n"
        << "    " << v.mt << " cm = kv_mrange(" << mask << ", plo, phi, ok);\n"
        << "    uint32_t kf = kv_mnz(cm) ? kv_mctz(cm) - " << u32(j) << " : 0u;\n"
        << "    bool found = kv_mnz(cm) & " << seg_expr(sg, "kf", false) << ";\n"
        << "    cm = kv_mpop(cm);\n"
        << "    if (!found && kv_mnz(cm)) {\n"
        << "      while (kv_mnz(cm)) {\n"
        << "        const uint32_t k = kv_mctz(cm) - " << u32(j) << "; cm = kv_mpop(cm);\n"
        << "        if (" << seg_expr(sg, "k", false) << ") { kf = k; found = true; break; }\n"
        << "      }\n"
        << "    }\n"
        << "    ok &= found;\n"
        << "    pos = kf + " << u32(sg.len) << "; }\n";
    }
    q << "  (void)pos; (void)end; (void)base;\n  return ok;\n}\n";
  }

  void qatom_fn(uint32_t ai, const QV& v) {
    if (!qatoms_done.insert({v.pfx, ai}).second) return;
    const Atom& A = ps.atoms[ai];
    atom_fn(ai);
    if (A.kind == AT_GLOB_E || A.kind == AT_GLOB_N) qglob_fn(ai, v);
    const std::string g = v.pfx + num("_glob_", ai);
    Helper o(*this, v.pfx + num("_atom_", ai));
    o << "__device__ __forceinline__ bool " << o.name << qsig(v) << " {\n";
    switch (A.kind) {
      case AT_GLOB_E:
        o << "  const bool r = " << g << "(w, lw, bm, n.c & NC_LEN_MASK, (n.c & NC_ASCII_E) != 0u, pstr);\n"
          << "  return (type != NT_MAP) & (type != NT_ARR) & (type != NT_NULL) & " << (A.op == CO_NE ? "!r" : "r") << ";\n";
        break;
      case AT_GLOB_N:
        o << "  if (type != NT_FLOAT && type != NT_MAP && type != NT_ARR && type != NT_BOOL && type != NT_NULL)\n"
          << "    return " << g << "(w, lw, bm, n.c & NC_LEN_MASK, (n.c & NC_ASCII_E) != 0u, pstr);\n"
          << "  return g_atom_" << ai << "(V, S, (const uint8_t*)lw, pstr, type, n);\n";
        break;
      default:
        o << "  return g_atom_" << ai << "(V, S, (const uint8_t*)lw, pstr, type, n);\n";
        break;
    }
    o << "}\n";
  }

  // the row's predicates on the register copy; non-string predicates are the g_pred ones
  void qpred_fn(uint32_t pi, const QV& v) {
    if (!qpreds_done.insert({v.pfx, pi}).second) return;
    const Pred& pr = ps.preds[pi];
    each_atom(pi, [&](uint32_t a) { qatom_fn(a, v); });
    Helper o(*this, v.pfx + num("_pred_", pi));
    o << "__device__ __forceinline__ bool " << o.name << qsig(v) << " {\n";
    if (pr.kind != PK_STRING) {
      o << "  return g_pred_" << pi << "(V, S, (const uint8_t*)lw, pstr, type, n);\n}\n";
      return;
    }
    // every alternative and conjunct evaluated (straight-line atoms), combined without branches
    o << "  return false";
    for (uint32_t a = pr.first; a < pr.first + pr.count; a++) {
      const Alt& al = ps.alts[a];
      o << "\n    | (true";
      for (uint32_t c = al.first; c < al.first + al.count; c++) {
        const Conj& cj = ps.conjs[c];
        auto call = [&](uint32_t at) {
          return std::string(1, v.pfx) + "_atom_" + std::to_string(at) + "(V, S, w, lw, bm, pstr, type, n)";
        };
        if (cj.kind == CJ_INRANGE) o << " & (" << call(cj.a0) << " & " << call(cj.a1) << ")";
        else if (cj.kind == CJ_NOTINRANGE) o << " & (" << call(cj.a0) << " | " << call(cj.a1) << ")";
        else o << " & " << call(cj.a0);
      }
      o << ")";
    }
    o << ";\n}\n";
  }

  // bytes whose masks the q_pred / r_pred of `pi` reads
  void pred_bytes(uint32_t pi, std::set<uint32_t>* out) const {
    each_atom(pi, [&](uint32_t at) {
      auto it = glob_bytes.find(at);
      if (it != glob_bytes.end()) out->insert(it->second.begin(), it->second.end());
    });
  }

  // ---------------------------------------------------------------- atoms / predicates
  void atom_fn(uint32_t ai) {
    if (!atoms_done.insert(ai).second) return;
    const Atom& A = ps.atoms[ai];
    if (A.kind == AT_GLOB_E || A.kind == AT_GLOB_N) glob_fn(ai);
    Helper o(*this, num("g_atom_", ai));
    o << "__device__ __forceinline__ bool " << o.name
      << "(const Val* __restrict__ V, const uint8_t* __restrict__ S, const uint8_t* __restrict__ E, "
         "const uint8_t* __restrict__ pstr, uint32_t type, const Node& n) {\n";
    switch (A.kind) {
      case AT_FALSE: o << "  return false;\n"; break;
      case AT_GLOB_E:
        o << "  if (type == NT_MAP || type == NT_ARR || type == NT_NULL) return false;\n"
          << "  const bool r = g_glob_" << ai << "(E, n.c & NC_LEN_MASK, (n.c & NC_ASCII_E) != 0u, pstr);\n"
          << "  return " << (A.op == CO_NE ? "!r" : "r") << ";\n";
        break;
      case AT_GLOB_N:
        o << "  if (type == NT_MAP || type == NT_ARR || type == NT_BOOL) return false;\n"
          << "  if (type == NT_NULL) return g_glob_" << ai << "(S, 1u, true, pstr);\n"
          << "  if (type != NT_FLOAT) return g_glob_" << ai << "(E, n.c & NC_LEN_MASK, (n.c & NC_ASCII_E) != 0u, pstr);\n"
          << "  const Val& v = V[n.a];\n"
          << "  return g_glob_" << ai << "(S + v.n_off, v.n_len, (v.flags & VF_ASCII_N) != 0u, pstr);\n";
        break;
      default: {  // AT_QCMP
        o << "  if (type == NT_MAP || type == NT_ARR || type == NT_BOOL) return false;\n"
          << "  int r;\n"
          << "  if (type == NT_NULL) {\n"
          << "    r = q_cmp(VF_Q_ZERO, 0, 0ull, 0ull, " << u32(A.q_flags) << ", " << A.q_exp << ", " << u64(A.q_hi) << ", "
          << u64(A.q_lo) << ");\n"
          << "  } else {\n"
          << "    const Val& v = V[n.a];\n"
          << "    if (!(v.flags & VF_Q_VALID)) return false;\n"
          << "    r = q_cmp(v.flags, v.q_exp, v.q_hi, v.q_lo, " << u32(A.q_flags) << ", " << A.q_exp << ", " << u64(A.q_hi)
          << ", " << u64(A.q_lo) << ");\n"
          << "  }\n"
          << "  return cmp_ok(" << u32(A.op) << ", r);\n";
        break;
      }
    }
    o << "}\n";
  }

  void pred_fn(uint32_t pi) {
    if (!preds_done.insert(pi).second) return;
    const Pred& pr = ps.preds[pi];
    each_atom(pi, [&](uint32_t a) { atom_fn(a); });
    // E: the validateString (e-form) bytes of the value, S + n.b in the rule kernels (a staged copy in kvj_ptab)
    Helper o(*this, num("g_pred_", pi));
    o << "__device__ __forceinline__ bool " << o.name
      << "(const Val* __restrict__ V, const uint8_t* __restrict__ S, const uint8_t* __restrict__ E, "
         "const uint8_t* __restrict__ pstr, uint32_t type, const Node& n) {\n";
    switch (pr.kind) {
      case PK_BOOL: o << "  return type == NT_BOOL && ((n.c & NC_BOOLV) != 0u) == " << (pr.flags ? "true" : "false") << ";\n"; break;
      case PK_FLOAT:
        o << "  if (type == NT_INT) return " << (pr.flags ? "V[n.a].i == " + i64(pr.fi) : std::string("false")) << ";\n"
          << "  if (type == NT_FLOAT) return V[n.a].f == " << f64(pr.f) << ";\n"
          << "  if (type == NT_STR) { const Val& v = V[n.a]; return (v.flags & VF_PF_OK) && v.f == " << f64(pr.f) << "; }\n"
          << "  return false;\n";
        break;
      case PK_NIL:
        o << "  if (type == NT_NULL) return true;\n"
          << "  if (type == NT_MAP || type == NT_ARR) return false;\n"
          << "  return (n.c & NC_NILLIKE) != 0u;\n";
        break;
      case PK_MAPTYPE: o << "  return type == NT_MAP;\n"; break;
      case PK_STRING: {
        for (uint32_t a = pr.first; a < pr.first + pr.count; a++) {
          const Alt& al = ps.alts[a];
          o << "  if (true";
          for (uint32_t c = al.first; c < al.first + al.count; c++) {
            const Conj& cj = ps.conjs[c];
            auto call = [&](uint32_t at) { return "g_atom_" + std::to_string(at) + "(V, S, E, pstr, type, n)"; };
            if (cj.kind == CJ_INRANGE) o << " && (" << call(cj.a0) << " && " << call(cj.a1) << ")";
            else if (cj.kind == CJ_NOTINRANGE) o << " && (" << call(cj.a0) << " || " << call(cj.a1) << ")";
            else o << " && " << call(cj.a0);
          }
          o << ") return true;\n";
        }
        o << "  return false;\n";
        break;
      }
      default: o << "  return false;\n"; break;
    }
    o << "}\n";
  }

  // memo slot of leaf predicate `pi` (one per predicate for single rules, assigned on first use)
  uint32_t slot_for(uint32_t pi) {
    auto it = pslot.find(pi);
    if (it != pslot.end()) return it->second;
    const uint32_t slot = (uint32_t)mpreds.size();
    mpreds.push_back(pi);
    pslot[pi] = slot;
    return slot;
  }
  // consecutive memo slots inside one table word for the leaf predicates of a rule group's
  // members (member j = bit base + j; a word's unused tail is padded with the first predicate)
  uint32_t group_slots(const std::vector<uint32_t>& preds) {
    if ((mpreds.size() % 32) + preds.size() > 32)
      while (mpreds.size() % 32) mpreds.push_back(preds[0]);
    const uint32_t base = (uint32_t)mpreds.size();
    for (uint32_t p : preds) mpreds.push_back(p);
    return base;
  }

  // Position classes of every leaf predicate: the projection-trie node of each
  // cursor is followed through the rule program (KEY: slot child, LOOP/EXIST/
  // INDEX: element node, keep-all scans: leaf-only positions, KEYGLOB: unknown),
  // and a predicate gets the class bit of every position it tests (its cursor,
  // and the element position when the value is an array). Ingest marks each
  // value with the class bits of the positions holding it (Val::cls), so the
  // table bit of (pred, value) is computed exactly when some node could read it.
  void leaf_classes(uint32_t ri) {
    // per cursor depth: projection-trie node (child lookups) and position id (value classes,
    // kv_pos_elem); -2 = unknown (every class)
    std::vector<int32_t> tn(8, -2), pos(8, -2);
    tn[0] = 0;
    pos[0] = 0;
    auto cls = [&](int32_t p) -> uint32_t { return p == -2 ? 0xFFFFFFFFu : kv_tcls(p); };
    auto epos = [&](int32_t p) -> int32_t { return p == -2 ? -2 : kv_pos_elem(p, 0); };
    for (uint32_t pc = ps.rules[ri].prog; pc < ps.prog.size(); pc++) {
      const Inst& in = ps.prog[pc];
      const uint32_t op = in.op & 0xFF, d = (in.op >> 8) & 0xFF, aux = (in.op >> 16) & 0xFF;
      if (op == OP_DONE) break;
      if (d + 2 > tn.size()) { tn.resize(d + 2, -2); pos.resize(d + 2, -2); }
      switch (op) {
        case OP_KEY:
        case OP_KEYV: {
          const int32_t t = tn[d];
          if (aux & AUX_SCAN) {  // children of keep-all maps: leaf-only positions
            tn[d + 1] = t == -2 ? -2 : -1;
            pos[d + 1] = t == -2 ? -2 : -1;
          } else if (t >= 0 && in.a < ps.trie.nodes[t].slot_keys.size()) {
            tn[d + 1] = pos[d + 1] = (int32_t)ps.trie.nodes[t].kids.at(ps.trie.nodes[t].slot_keys[in.a]);
          } else {
            tn[d + 1] = pos[d + 1] = -2;
          }
          break;
        }
        case OP_KEYGLOB: {  // a resolved label / annotation key: a child of a keep-all map (pos -1)
          const int32_t t = tn[d];
          tn[d + 1] = pos[d + 1] = t >= 0 && ps.trie.nodes[t].keep_all ? -1 : -2;
          break;
        }
        case OP_LOOP_BEGIN:
        case OP_EXIST_BEGIN:
        case OP_INDEX:
          tn[d + 1] = tn[d] >= 0 ? ps.trie.nodes[tn[d]].elem : tn[d];
          pos[d + 1] = epos(pos[d]);
          break;
        case OP_LEAF: pmask[in.a] |= cls(pos[d]) | cls(epos(pos[d])); break;
        default: break;
      }
    }
  }

  // kvj_ptab: one lane per distinct scalar Val of the batch; evaluates every memo
  // slot's predicate on the scalar node ingest builds for that value
  // (kvingest.cpp scalar(): a = val id, b = e_off, c = e_len | NC_* flags)

  // the slots `ks` by predicate (a predicate holds several slots when rule groups share it):
  // predicate -> (table word -> bits), in first-slot order
  std::vector<std::pair<uint32_t, std::map<uint32_t, uint32_t>>> pred_words(const std::vector<uint32_t>& ks) const {
    std::vector<std::pair<uint32_t, std::map<uint32_t, uint32_t>>> out;
    std::map<uint32_t, size_t> at;
    for (uint32_t k : ks) {
      auto it = at.find(mpreds[k]);
      if (it == at.end()) {
        it = at.emplace(mpreds[k], out.size()).first;
        out.push_back({mpreds[k], {}});
      }
      out[it->second].second[k / 32] |= 1u << (k % 32);
    }
    return out;
  }

  // predicates per kvj_ptab thread: all of them (one grid row)
  uint32_t ptab_row_out() const { return std::max<uint32_t>(1u, (uint32_t)mpreds.size()); }

  void ptab_kernel() {
    // register-path predicates (helpers: emitted before the kernel text)
    for (uint32_t k = 0; k < mpreds.size(); k++) qpred_fn(mpreds[k], kQ64);
    for (uint32_t k = 0; k < mpreds.size(); k++) qpred_fn(mpreds[k], kQ128);
    std::ostringstream o;
    const uint32_t nw = (uint32_t)((mpreds.size() + 31) / 32);
    auto pm = [&](uint32_t k) { auto it = pmask.find(mpreds[k]); return it == pmask.end() ? 0xFFFFFFFFu : it->second; };
    // predicates grouped by position class: a value runs the groups its class bits select
    // (Vals are numbered by class, kvingest.cpp val_order_key, so the tests are uniform in
    // most waves); one thread per value writes every word of its table column
    std::map<uint32_t, std::vector<uint32_t>> groups;  // class mask -> memo slots
    uint32_t all = 0;
    for (uint32_t k = 0; k < mpreds.size(); k++) {
      groups[pm(k)].push_back(k);
      all |= pm(k);
    }
    o << "extern \"C\" __global__ __launch_bounds__(KV_WG) void kvj_ptab(const DevPS* __restrict__ Pp, "
         "const Val* __restrict__ V, const uint8_t* __restrict__ S, uint32_t NV, uint32_t* __restrict__ PT) {\n"
      << "  const uint32_t v = blockIdx.x * KV_WG + threadIdx.x;\n"
      << "  const uint32_t NP = NV + KV_PTAB_PSEUDO;  // table pitch\n"
      << "  if (v >= NP) return;\n"
      << "  uint32_t w[" << nw << "] = {};\n"
      << "  if (v >= NV) {  // pseudo columns: every predicate on a null / map / array node\n"
      << "    const uint8_t* __restrict__ pstr = Pp->pstr;\n"
      << "    const uint32_t type = v == NV ? NT_NULL : v == NV + 1u ? NT_MAP : NT_ARR;\n"
      << "    const Node n{type, 0u, 0u, 0u};\n";
    {
      std::vector<uint32_t> all_k(mpreds.size());
      for (uint32_t k = 0; k < mpreds.size(); k++) all_k[k] = k;
      for (const auto& [pi, wb] : pred_words(all_k)) {
        o << "    if (g_pred_" << pi << "(V, S, S, pstr, type, n)) {";
        for (const auto& [wi, bits] : wb) o << " w[" << wi << "] |= " << u32(bits) << ";";
        o << " }\n";
      }
    }
    for (uint32_t i = 0; i < nw; i++) o << "    PT[(size_t)" << i << "u * NP + v] = w[" << i << "];\n";
    o << "    return;\n  }\n"
      << "  const uint32_t vc = V[v].cls;\n"
      << "  if (vc & " << u32(all) << ") {\n"
      << "  const uint8_t* __restrict__ pstr = Pp->pstr;\n"
      << "  const Val& val = V[v];\n"
      << "  const uint32_t type = val.type;\n"
      << "  Node n{type, v, val.e_off, val.e_len};\n"
      << "  if (val.flags & VF_ASCII_E) n.c |= NC_ASCII_E;\n"
      << "  if (val.flags & VF_BOOLV) n.c |= NC_BOOLV;\n"
      << "  if (val.flags & VF_NILLIKE) n.c |= NC_NILLIKE;\n"
      << "  const uint8_t* __restrict__ E = S + val.e_off;\n"
      // values of <= 64 (<= 128) bytes: 16 (32) words in registers (loads clamped to the
      // word after the string, which the word-wise readers already touch) and an LDS copy of
      // 33 words (odd stride: no bank conflicts) for the reads at a per-lane offset; values
      // are numbered by length bucket within their class, so a wave runs one of the paths
      << "  __shared__ uint32_t lds_e[KV_WG * 33];\n"
      << "  uint32_t* lw = lds_e + threadIdx.x * 33u;\n";
    for (const QV* qv : {&kQ64, &kQ128}) {
      const uint32_t W = qv->words;
      o << (W == 16 ? "  if (val.e_len <= 64u) {\n" : "  } else if (val.e_len <= 128u) {\n")
        << "    uint32_t sw[" << W << "];\n"
        << "    const uint32_t* __restrict__ src = (const uint32_t*)E;\n"
        << "    const uint32_t lastw = (val.e_len + 3u) >> 2;\n"
        << "#pragma unroll\n"
        << "    for (uint32_t i = 0; i < " << W << "u; i++) sw[i] = src[i < lastw ? i : lastw];\n"
        << "#pragma unroll\n"
        << "    for (uint32_t i = 0; i < " << W << "u; i++) lw[i] = sw[i];\n"
        << "    lw[" << W << "] = src[lastw];\n"
        // byte masks only over the words the wave's values occupy
        << "    const uint32_t nwu_ = kv_wave_words(lastw, " << W << "u);\n";
      for (auto& [m, ks] : groups) {
        std::set<uint32_t> bytes;
        for (uint32_t k : ks) pred_bytes(mpreds[k], &bytes);
        o << "    if (vc & " << u32(m) << ") {\n";
        if (!bytes.empty()) {
          o << "      " << qv->mt << " bm[" << kMaxBSlots << "];\n";
          for (uint32_t c : bytes)
            o << "      bm[" << bslot.at(c) << "] = " << qv->bmk << "_n(sw, " << hex32(c * 0x01010101u) << ", nwu_);\n";
        } else {
          o << "      const " << qv->mt << "* bm = nullptr;\n";
        }
        for (const auto& [pi, wb] : pred_words(ks)) {  // each predicate once, into every slot it has
          o << "      { const bool p_ = " << qv->pfx << "_pred_" << pi << "(V, S, sw, lw, bm, pstr, type, n);";
          for (const auto& [wi, bits] : wb) o << " w[" << wi << "] |= p_ ? " << u32(bits) << " : 0u;";
          o << " }\n";
        }
        o << "    }\n";
      }
    }
    o << "  } else {\n";
    for (auto& [m, ks] : groups) {
      o << "    if (vc & " << u32(m) << ") {\n";
      for (const auto& [pi, wb] : pred_words(ks)) {
        o << "      if (g_pred_" << pi << "(V, S, E, pstr, type, n)) {";
        for (const auto& [wi, bits] : wb) o << " w[" << wi << "] |= " << u32(bits) << ";";
        o << " }\n";
      }
      o << "    }\n";
    }
    o << "  }\n  }\n";
    for (uint32_t i = 0; i < nw; i++) o << "  PT[(size_t)" << i << "u * NP + v] = w[" << i << "];\n";
    o << "}\n\n";
    kernels.push_back({"kvj_ptab", o.str()});
  }

  // dynamic leaves (pattern variables, kvvars.cpp): the generic predicate evaluator on the
  // batch table, out of line (one copy per program; inlined per leaf it multiplies the
  // kernel's code and its compile time). One record: the wrapper every VLEAF calls, and the
  // evaluator it reaches (declared in the prelude), so a program that takes one takes both.
  void dleaf_fn() {
    if (dleaf_done) return;
    dleaf_done = true;
    Helper o(*this, "g_dleaf_0");
    o << "__device__ __forceinline__ bool g_dleaf_0(const DevBatch& B, const Node* __restrict__ N, uint32_t dp, "
         "const Node& vn) { return kv_dleaf_impl(B, N, dp, vn); }\n"
      << "__device__ __noinline__ bool kv_dleaf_impl(const DevBatch& B, const Node* __restrict__ N, uint32_t dp, Node vn) {\n"
      << "  const uint32_t vt = node_type(vn.kt);\n"
      << "  if (vt == NT_ARR) {\n"
      << "    for (uint32_t k = 0; k < vn.b; k++) if (!pred_node(*B.dps, B, N, dp, ni(vn.a + k))) return false;\n"
      << "    return true;\n  }\n"
      << "  return pred_eval(*B.dps, B, dp, vt, vn);\n}\n";
  }

  // ---------------------------------------------------------------- match / exclude
  // blk_ok(f) == !(MF_EMPTY) && doesResourceMatchConditionBlock(f) has no errors
  // (pkg/engine/utils.go:265-336); MF_EMPTY / MF_UI_FAIL are folded per launch
  // (user info), so they are read from P.fflags; every other criterion is static.
  void blk_fn(uint32_t f) {
    if (!blks_done.insert(f).second) return;
    const MFilter& F = ps.filters[f];
    for (uint32_t a : ps.filter_name_atoms.at(f)) glob_fn(a);  // before this function's text
    Helper o(*this, num("g_blk_", f));
    o << "__device__ __forceinline__ bool " << o.name
      << "(const DevPS& P, const DevBatch& B, const Res* __restrict__ R, uint32_t rkind, uint32_t rflags) {\n"
      << "  if (sld(P.fflags + " << f << "u) & (MF_EMPTY | MF_UI_FAIL)) return false;\n";
    if (F.flags & MF_KINDS) {
      bool any_star = false;
      std::ostringstream k;
      k << "false";
      for (uint32_t i = F.kinds_first; i < F.kinds_first + F.kinds_count; i++) {
        const KindSpec& ks = ps.kinds[i];
        switch (ks.form) {
          case 3: any_star = true; break;
          case 0: k << " || rkind == " << u32(ks.kind); break;
          case 1: k << " || (rkind == " << u32(ks.kind) << " && R->version == " << u32(ks.version) << ")"; break;
          default:
            k << " || (R->group == " << u32(ks.group) << " && rkind == " << u32(ks.kind) << " && (R->version == "
              << u32(ks.version) << " || R->version == P.star_id))";
            break;
        }
      }
      if (!any_star) o << "  if (!(" << k.str() << ")) return false;\n";
    }
    // name / names: compiled word globs over the resource name (no calls)
    const std::vector<uint32_t>& na = ps.filter_name_atoms.at(f);
    auto name_glob = [&](uint32_t a) {
      return "g_glob_" + std::to_string(a) + "(B.bstr + R->name_off, R->name_len, (rflags & RF_NAME_ASCII) != 0u, P.pstr)";
    };
    size_t k = 0;
    if (F.flags & MF_NAME) o << "  if (!" << name_glob(na.at(k++)) << ") return false;\n";
    if (F.flags & MF_NAMES) {
      o << "  if (!(false";
      for (; k < na.size(); k++) o << " || " << name_glob(na[k]);
      o << ")) return false;\n";
    }
    // namespace globs, annotations, label selectors: bits of the pass's match tables (kv_mtab)
    if (F.flags & MF_NSS) o << "  if (!mt_bit(P.mt_ns, " << u32(F.nss_bit) << ", B.n_nsm, R->nsm)) return false;\n";
    if (F.flags & MF_ANN) o << "  if (!mt_bit(P.mt_ann, " << u32(F.ann_bit) << ", B.n_asets, R->aset)) return false;\n";
    if (F.flags & MF_SEL) o << "  if (!mt_bit(P.mt_sel, " << u32(F.sel) << ", B.n_lsets, R->lset)) return false;\n";
    if (F.flags & MF_NSSEL)
      o << "  if (!(rflags & (RF_KIND_NAMESPACE | RF_KIND_EMPTY)) && !((B.ns_bits[R->ns_index * B.ns_words + "
        << (F.nssel_bit / 32) << "u] >> " << (F.nssel_bit % 32) << "u) & 1u)) return false;\n";
    o << "  return true;\n}\n";
  }

  // rule_matches (kvdevfn.h) for one rule, with its filter list unrolled
  void match_fn(uint32_t ri) {
    const RuleRec& rr = ps.rules[ri];
    for (uint32_t f = rr.m_first; f < rr.m_first + rr.m_count; f++) blk_fn(f);
    for (uint32_t f = rr.x_first; f < rr.x_first + rr.x_count; f++) blk_fn(f);
    auto call = [&](uint32_t f) { return "g_blk_" + std::to_string(f) + "(P, B, R, rkind, rflags)"; };
    auto combine = [&](uint32_t mode, uint32_t first, uint32_t count) {
      std::ostringstream e;
      if (mode == 0 || count == 0) {
        e << call(first);
      } else {
        e << "(";
        for (uint32_t f = first; f < first + count; f++) e << (f > first ? (mode == 1 ? " || " : " && ") : "") << call(f);
        e << ")";
      }
      return e.str();
    };
    Helper o(*this, num("g_match_", ri));
    o << "__device__ __forceinline__ bool " << o.name
      << "(const DevPS& P, const DevBatch& B, const Res* __restrict__ R, uint32_t rkind, uint32_t rflags) {\n"
      << "  if (!" << combine(rr.m_mode, rr.m_first, rr.m_count) << ") return false;\n"
      << "  return !" << combine(rr.x_mode, rr.x_first, rr.x_count) << ";\n}\n";
  }

  // ---------------------------------------------------------------- rule programs
  static uint32_t prog_end(const PolicySet& ps, uint32_t pc) {
    while ((ps.prog[pc].op & 0xFF) != OP_DONE) pc++;
    return pc;
  }

  // ================================================================ fused chunk kernels
  // All rules of a chunk run in one kernel body as interleaved sequential
  // programs. Rules never interact, so any interleaving that keeps each rule's
  // own op order is exact; the interleaving is chosen to share memory traffic:
  //  * cursor lookups whose path from the resource root (or from the element
  //    of a shared array loop) is known statically are hoisted: computed once
  //    (per kernel, or per loop iteration), just before the first rule that
  //    walks them, together with the 16-B node they land on;
  //  * every rule program is split at its top-level array loops into stages;
  //    at stage k the k-th loops of all rules iterating the same array
  //    (e.g. spec.containers) become ONE loop whose body runs each active
  //    rule's loop body for that element.
  // Per-rule registers: rs (resume pc between stages | ACTIVE bit, or FIN |
  // status once the rule's DONE ran), ek (error kind | flags << 4 | pattern
  // node << 8), loop indices of the raise (ei0..), anchor bitsets when used.
  static constexpr uint32_t FIN = 0x7F000000u, ACT = 0x80000000u;

  // Leaves on a hoisted node read their table word(s) through a load hoisted with the cursor
  // instead of one dependent load per rule. A hoist region (the root table of a block, the
  // element table of a fused loop) is emitted at the top of its block stage / loop body, in one
  // of two layouts per kernel (HoistTable::flush, JitKernelPlan::grouped). First-use order:
  // cells and words as the rules ask for them, each word with its array case inline; every
  // word's branch cuts the loads behind it off from the ones before. Three parts: every
  // path-column cell load with its index select, then every table-word gather, then one fix-up
  // for leaf cells that are arrays; the first two have no branch, so the compiler is free to
  // issue the cell loads together and the gathers together (what it does with that, loop by
  // loop: DESIGN.md section 4, Hoist regions). It needs more registers, so a kernel keeps it
  // only if it fits at the plan made in first-use order (kvjitbuild.cpp jit_group_regions).
  //
  // hoisted cursor: node index var + Node var, and the path column the node is read from
  // (fam -1: none). The index var of a column's node is a node index for a map only.
  struct HVar {
    std::string idx, node;
    int fam = -1;
    uint32_t j = kNoCol;
  };
  struct HWord {  // table word `word` of the leaf on hoisted node `hv`, in variable `var`
    std::string var;
    HVar hv;
    uint32_t word = 0;
  };
  struct HoistTable {
    std::string prefix;
    std::map<std::string, HVar> vars;
    // the lookups, one statement group per entry, in call order (a walk of the node rows stays
    // behind the cell it starts from), and the leaf words on them, in order of first use
    std::vector<std::string> cells;
    std::vector<HWord> words;
    std::vector<char> order;     // first-use order of both: 'c' the next cell, 'w' the next word
    std::set<std::string> have;  // (the words' variables)
    size_t cflushed = 0, wflushed = 0, oflushed = 0;
    void add_cell(const std::string& c) { cells.push_back(c); order.push_back('c'); }
    void add_word(const HWord& w) { words.push_back(w); order.push_back('w'); }
    uint32_t n = 0;
    // path columns: the family its lookups read (-1: none, walk the node rows), the root token
    // of its exprs (an element family) and the word offset of its lane's row in the pool
    int fam = -1;
    std::string troot, cell0;
    // an empty asm statement with the words `xs` as inputs: their loads are issued, together, ahead of it
    static std::string joined(const std::vector<std::string>& xs) {
      std::string s;
      for (size_t i = 0; i < xs.size(); i += 8) {  // (a few inputs per statement)
        s += "#ifndef KVEMU\n  asm volatile(\"\" ::";
        for (size_t k = i; k < xs.size() && k < i + 8; k++) s += (k > i ? ", \"v\"(" : " \"v\"(") + xs[k] + ")";
        s += ");\n#endif\n";
      }
      return s;
    }
    // What was hoisted since the last flush. grouped: in three parts, the cell loads, the gathers
    // of the leaf words (kv_leaf_gather: no branch, so they issue behind the cell loads' one wait),
    // and the fix-up of the words whose cell is an array (kv_leaf_fix), under one wave-uniform
    // test. Otherwise in first-use order, each word whole (kv_leaf_word: its array case inline).
    // join (three parts only; a column loop's region, flushed once): the words `join` and the
    // region's cell words, then its gathered words, are `joined` behind their part, so every load
    // of a part is issued ahead of the first branch that reads one of them (left alone the
    // compiler sinks a cell's load below the test of the cell before it).
    std::string flush(bool grouped, const std::vector<std::string>* join = nullptr) {
      std::string s;
      if (!grouped) {
        for (; oflushed < order.size(); oflushed++) {
          if (order[oflushed] == 'c') {
            s += cells[cflushed++];
            continue;
          }
          const HWord& x = words[wflushed++];
          s += "  const uint32_t " + x.var + " = " +
               (x.hv.fam >= 0 ? col_macro("LO", (uint32_t)x.hv.fam, x.hv.j) : std::string("KVC_LO_ROW")) + "(" + x.hv.node +
               ", " + std::to_string(x.word) + "u);\n";
        }
        return s;
      }
      oflushed = order.size();
      for (; cflushed < cells.size(); cflushed++) s += cells[cflushed];
      if (join) {
        std::vector<std::string> xs = *join;
        for (const auto& kv : vars)
          if (kv.second.fam >= 0) xs.push_back(kv.second.node + ".kt");
        s += joined(xs);
      }
      if (wflushed == words.size()) return s;
      std::vector<std::string> nodes;  // the words' nodes, each once
      std::string fix;
      for (size_t i = wflushed; i < words.size(); i++) {
        const HWord& x = words[i];
        const bool col = x.hv.fam >= 0;
        const std::string args = "(" + x.hv.node + ", " + std::to_string(x.word) + "u);\n";
        s += "  uint32_t " + x.var + " = " + (col ? col_macro("LW", (uint32_t)x.hv.fam, x.hv.j) : std::string("KVC_LW_ROW")) + args;
        if (std::find(nodes.begin(), nodes.end(), x.hv.node) == nodes.end()) nodes.push_back(x.hv.node);
        fix += "    if (node_type(" + x.hv.node + ".kt) == NT_ARR) " + x.var + " = " +
               (col ? col_macro("LA", (uint32_t)x.hv.fam, x.hv.j) : std::string("KVC_LA_ROW")) + args;
      }
      if (join) {
        std::vector<std::string> xs;
        for (size_t i = wflushed; i < words.size(); i++) xs.push_back(words[i].var);
        s += joined(xs);
      }
      wflushed = words.size();
      s += "  if (__ballot(";
      for (size_t i = 0; i < nodes.size(); i++) s += (i ? " || " : "") + ("node_type(" + nodes[i] + ".kt) == NT_ARR");
      return s + ") != 0ull) {  // some leaf cell is an array (rare)\n" + fix + "  }\n";
    }
  };

  struct RGen {  // per-rule generation state
    uint32_t ri = 0, b = 0, e = 0, maxd = 1;
    std::vector<std::pair<uint32_t, uint32_t>> loops;  // stage loops (LOOP_BEGIN pc, LOOP_END pc)
    std::vector<std::string> expr;                      // symbolic cursor per depth ("" = unknown)
    std::vector<HVar> hv;                               // hoisted vars per depth (when expr known)
    // per depth: the columns whose index var was assigned to the rule's cursor c<d> (a use of the
    // cursor as a node index makes them all wide)
    std::vector<std::vector<std::pair<int, uint32_t>>> csrc;
    std::set<uint32_t> resume;                          // resume targets of later segments
    // resume targets set by earlier stages and not consumed yet (the segment holding them lies
    // further on), reached without / with a pending error
    std::set<uint32_t> carry_ok, carry_err;
    // per stage loop k: the rule is "lean" there (its state is one bit of the block's stage-k
    // masks and a failing element decides its status at once), the status its post chain adds
    // to the error (flags), whether that chain ends at the last anyPattern alternative, and the
    // one target past the loop that the stage-k segment jumps to (0xFFFFFFFF: none)
    std::vector<char> lean, post_alt;
    std::vector<uint32_t> post_flags, skip_to;
    uint32_t q = 0;                                     // position in the block (mask bit, LDS row)
    bool uses_anchor = false, uses_keyglob = false;
    // rule group: the representative's program run once for all members (bit j of `al` = member
    // j alive on this lane); every error is decided where it is raised (kv_gfin)
    bool grp = false;
    uint32_t gn = 1, grow = 0, gsri = 0, gspn = 0;      // members, LDS row of member 0, steps
    std::vector<uint32_t> gri, gdpn;                    // member rule ids, pattern-node shifts
    std::map<uint32_t, uint32_t> gslot;                 // representative LEAF pc -> slot of member 0
    std::string gtab;                                   // member table (empty: arithmetic)
    bool gsite = false;                                 // site records (gl: its counter in the kernel)
    uint32_t gl = 0, gpre = 0;
    uint32_t max_level = 0;
    std::string s;                                      // "_<ri>"
  };

  HVar hoist(HoistTable& T, const std::string& pexpr, const HVar& p, uint32_t a, uint32_t aux) {
    const bool scan = (aux & AUX_SCAN) != 0;
    const std::string ex = pexpr + (scan ? "/k" : "/s") + std::to_string(a);
    auto it = T.vars.find(ex);
    if (it != T.vars.end()) return it->second;
    HVar h{T.prefix + "h" + std::to_string(T.n), T.prefix + "hn" + std::to_string(T.n)};
    T.n++;
    std::ostringstream c;
    const uint32_t j = T.fam >= 0 ? col_of((uint32_t)T.fam, T.fam == 0 ? ex : ex.substr(T.troot.size())) : kNoCol;
    if (j != kNoCol) {
      // the node from its path column (absent: the zero cell); the index only where the
      // lookup's presence (or a map's own index: wildcard keys) is asked for
      h.fam = T.fam;
      h.j = j;
      c << "  const Node " << h.node << " = " << col_macro("LD", (uint32_t)T.fam, j) << "(" << T.cell0 << ");\n"
        << "  const uint32_t " << h.idx << " = " << h.node << ".kt == 0u ? ABSENT : "
        << col_macro("IX", (uint32_t)T.fam, j) << "(" << h.node << ");\n";
      T.add_cell(c.str());
      T.vars.emplace(ex, h);
      return h;
    }
    col_mark(p.fam, p.j, CU_WIDE | CU_B);  // the walk below reads the parent's a and b
    c << "  uint32_t " << h.idx << " = ABSENT; Node " << h.node << "{0u, 0u, 0u, 0u};\n";
    if (scan) {
      c << "  if (node_type(" << p.node << ".kt) == NT_MAP) for (uint32_t q_ = 0u; q_ < " << p.node << ".b; q_++) { "
        << "const uint32_t c_ = ni(" << p.node << ".a + q_); const Node t_ = N[c_]; if (node_key(t_.kt) == " << u32(a)
        << ") { " << h.idx << " = c_; " << h.node << " = t_; break; } }\n";
    } else {
      // the loaded node passes through v_perm (keep / zero) instead of a select,
      // which the compiler would turn into a branch around a narrowed reload
      c << "  { const bool ok_ = node_type(" << p.node << ".kt) == NT_MAP && " << u32(a) << " < " << p.node << ".b; "
        << "const uint32_t c_ = ok_ ? ni(" << p.node << ".a + " << u32(a) << ") : 0u; const Node t_ = N[c_]; "
        << "const bool hit_ = ok_ && node_type(t_.kt) != NT_ABSENT; const uint32_t m_ = hit_ ? 0x07060504u : 0x0c0c0c0cu; "
        << h.idx << " = hit_ ? c_ : ABSENT; " << h.node << " = Node{__builtin_amdgcn_perm(t_.kt, 0u, m_), "
        << "__builtin_amdgcn_perm(t_.a, 0u, m_), __builtin_amdgcn_perm(t_.b, 0u, m_), __builtin_amdgcn_perm(t_.c, 0u, m_)}; }\n";
    }
    T.add_cell(c.str());
    T.vars.emplace(ex, h);
    return h;
  }

  // a region of one rule's program: a segment between stage loops (kind 0) or
  // the body of a fused loop (kind 1)
  struct Region {
    int kind = 0;
    uint32_t rb = 0, re = 0;  // ops emitted: [rb, re)
    uint32_t jre = 0;         // local jump targets: [rb, jre)
    std::string se;           // segment end label
    // out (kind 0): the targets past the segment that it jumps to, without / with a pending error
    std::set<uint32_t>*jumps = nullptr, *err_jumps = nullptr;
    std::string li0;          // level-0 loop index expression
    HoistTable* T = nullptr;  // hoist table for exprs rooted at this region's loop element
    std::string troot;        // expr root of T
  };

  // Rule groups: rules of one structural form (group_form) whose pattern nodes differ by one
  // constant run the representative's program once, with one bit per member; their leaf predicates
  // take consecutive bits of one table word, so a leaf tests every member with one shift and mask.
  struct GInfo {
    std::vector<uint32_t> members, pns0, leafpcs;
    std::vector<uint32_t> dpn;                 // pattern-node shift of each member
    std::vector<std::vector<uint32_t>> preds;  // leaf predicates of each member
  };

  // One fused block of a kernel while it is generated (fused_block owns it): its rules in block
  // position order (a group's members take consecutive positions, at its first member's place),
  // their status rows [hbase, hbase + rules) of the kernel's LDS (KV_RSTRIDE bytes each), the
  // generation state of every rule that runs a program (a group: its representative's), and the
  // hoist table of the lookups from the resource root.
  struct Block {
    Kern& kern;
    const uint32_t hbase;
    std::vector<uint32_t> rules;
    std::vector<GInfo> ginfo;
    std::map<uint32_t, size_t> gof;  // rule -> group
    std::vector<RGen> gs;
    HoistTable global;
    size_t K = 0;  // stage loops of its deepest rule
    Block(Kern& k, uint32_t hb) : kern(k), hbase(hb) {
      global.prefix = "g";
      global.fam = 0;
      global.cell0 = "gw_";
    }
    uint32_t mask_words() const { return ((uint32_t)rules.size() + 31) / 32; }
    // the generation state of the rule (or group representative) at block position q, if it has one
    const RGen* at(uint32_t q) const {
      for (const RGen& x : gs)
        if (x.q == q) return &x;
      return nullptr;
    }
    // the group whose representative `ri` is (nullptr: no group); member: `ri` is a later member
    const GInfo* group_of(uint32_t ri, bool* member) const {
      auto it = gof.find(ri);
      *member = it != gof.end() && ginfo[it->second].members[0] != ri;
      return it == gof.end() ? nullptr : &ginfo[it->second];
    }
  };

  // A per-rule loop (an existence anchor, a loop nested in a loop element) over an array that is
  // a path column: its elements are the rows of the array's family (a nested family when the
  // array lies in a loop element), and the lookups and leaves below an element are a hoist region
  // of their own at the head of the loop body, so the body is emitted once its END is reached:
  //   { uint32_t <row offset>; <BEGIN> <body label>:; <element cell> <region> <body> <END> }
  // The braces keep the region's declarations out of the scope of every jump past the loop.
  struct ColLoop {
    uint32_t body_pc = 0, end_pc = 0, fam = 0;
    std::string troot;
    HoistTable T;
    std::ostringstream body;
    std::ostream* outer = nullptr;
  };

  void emit_region(Block& B, RGen& g, const Region& R, std::ostream& w0) {
    const std::string& s = g.s;
    std::list<ColLoop> cloops;  // the open ones, innermost last
    std::ostream* wcur = &w0;
    auto cloop_of = [&](const std::string& ex) -> ColLoop* {
      for (auto it = cloops.rbegin(); it != cloops.rend(); ++it) {
        const size_t n = it->troot.size();
        if (ex.compare(0, n, it->troot) == 0 && (ex.size() == n || ex[n] == '/')) return &*it;
      }
      return nullptr;
    };
    auto C = [&](uint32_t d) { return "c" + std::to_string(d) + s; };
    auto L = [&](uint32_t pc) { return "R" + std::to_string(g.ri) + "_L" + std::to_string(pc); };
    // err: the jump carries a pending error (a raise, or an error passed on by a scope end)
    auto jump = [&](uint32_t t, bool err = false) -> std::string {
      if (t >= R.rb && t < R.jre) return "goto " + L(t) + ";";
      if (R.kind == 0 && t >= R.jre) {
        g.resume.insert(t);
        (err ? R.err_jumps : R.jumps)->insert(t);
        return "{ rs" + s + " = " + u32(t) + "; goto " + R.se + "; }";
      }
      throw std::runtime_error("kvjit: jump out of a fused region (rule " + std::to_string(g.ri) + ")");
    };
    auto finish = [&](const std::string& st) {
      if (R.kind != 0) throw std::runtime_error("kvjit: rule end inside a fused loop");
      return "{ rs" + s + " = FIN_ | " + st + "; goto " + R.se + "; }";
    };
    auto li = [&](uint32_t lv) { return lv == 0 && R.kind == 1 ? R.li0 : "li" + std::to_string(lv) + s; };
    const bool G = g.grp;
    const std::string al = "al" + s;
    // a group with no member left on this lane leaves the region
    auto gdone = [&]() -> std::string {
      if (R.kind == 0) return "{ rs" + s + " = FIN_ | ST_STORED_; goto " + R.se + "; }";
      return "goto " + L(R.re) + ";";
    };
    // members `m` of a group fail with the representative's error (kind, pn) raised here: their
    // status is the error's, carried statically through the scope ends to DONE (post_chain)
    auto gfin = [&](const std::string& m, uint32_t kind, uint32_t pn, uint32_t catch_pc) {
      const PostChain pcn = post_chain(g, catch_pc);
      if (!pcn.pure || pcn.alt) throw std::runtime_error("kvjit: impure error chain in rule group");
      std::string st;
      if (kind == E_CPU) st = "ST_CPU";
      else if (pcn.flags & (EF_COND | EF_GLOBAL)) st = "ST_SKIP";
      else {
        st = kind == E_LEN ? "ST_ERROR" : "ST_FAIL";
        if (g.uses_anchor) st = "((areg" + s + " & ~apres" + s + ") ? ST_ERROR : " + st + ")";
      }
      std::ostringstream r;
      r << "kv_gfin<" << (g.gtab.empty() ? "false" : "true") << ", " << (g.gsite ? "true" : "false")
        << ">(O, n_res, r, valid, " << m << ", " << st << ", " << u32(kind | (pcn.flags << 4) | (pn << 8));
      for (uint32_t lv = 0; lv < 4; lv++) r << ", " << (lv <= g.max_level ? li(lv) : std::string("0u"));
      r << ", s_w + " << u32(KV_ROW0 + g.grow * KV_RSTRIDE) << ", " << u32(g.grow) << ", " << (g.gtab.empty() ? std::string("nullptr") : g.gtab) << ", "
        << u32(g.gn) << ", " << u32(g.gri[0]) << ", " << u32(g.gsri) << ", " << u32(g.gspn) << ", "
        << (!g.gsite && g.gn >= kGslotMembers ? "true" : "false");
      if (g.gsite) r << ", s_gc_ + " << u32(KV_RWAVES * g.gl) << ", " << u32(g.gpre);
      r << ");";
      return r.str();
    };
    auto raise = [&](uint32_t kind, uint32_t pn, uint32_t catch_pc) {
      if (pn >= (1u << 24)) throw std::runtime_error("kvjit: pattern node id exceeds 24 bits");
      if (G) return "{ " + gfin(al, kind, pn, catch_pc) + " " + al + " = 0u; " + gdone() + " }";
      std::ostringstream r;
      r << "{ ek" << s << " = " << u32(kind) << " | " << u32(pn << 8) << ";";
      for (uint32_t lv = 0; lv <= g.max_level && lv < 4; lv++) r << " ei" << lv << s << " = " << li(lv) << ";";
      if (g.uses_keyglob) r << " ekn" << s << " = kn" << s << ";";
      r << " " << jump(catch_pc, true) << " }";
      return r.str();
    };
    auto known = [&](uint32_t d) {
      if (d >= g.expr.size() || g.expr[d].empty()) return false;
      const std::string& ex = g.expr[d];
      return ex[0] == 'R' || (R.T && ex.compare(0, R.troot.size(), R.troot) == 0) || cloop_of(ex);
    };
    // the cursor c<d> read as a node index: the columns it may come from hold one (wide)
    auto IDX = [&](uint32_t d) {
      if (d < g.csrc.size())
        for (const auto& cj : g.csrc[d]) col_mark(cj.first, cj.second, CU_WIDE);
    };
    // the node at depth d; `use`: what is read of it beyond its type (ColUse)
    auto NODE = [&](uint32_t d, uint32_t use = 0u) -> std::string {
      if (known(d)) {
        col_mark(g.hv[d].fam, g.hv[d].j, use);
        return g.hv[d].node;
      }
      IDX(d);
      return "N[" + C(d) + "]";
    };
    auto table_for = [&](uint32_t d) -> HoistTable* {
      const std::string& ex = g.expr[d];
      if (ex[0] == 'R') return &B.global;
      if (R.T && ex.compare(0, R.troot.size(), R.troot) == 0) return R.T;
      if (ColLoop* cl = cloop_of(ex)) return &cl->T;
      return nullptr;
    };
    // "the node at depth d is absent or its type <cmp>": a hoisted node carries its absence as
    // type 0; otherwise the cursor is tested before the node it points at is read
    auto absent_or = [&](uint32_t d, const char* cmp) {
      const std::string test = "node_type(" + NODE(d) + ".kt) " + cmp;
      return known(d) ? test : C(d) + " == ABSENT || " + test;
    };
    auto set_unknown = [&](uint32_t from) {
      for (uint32_t x = from; x < g.expr.size(); x++) g.expr[x].clear();
    };
    // key lookup: returns the index expression; records the child cursor expr at d+1 when assign
    auto lookup = [&](uint32_t d, uint32_t a, uint32_t aux, bool assign) -> std::string {
      const uint32_t laux = aux & AUX_SCAN;
      HoistTable* T = known(d) ? table_for(d) : nullptr;
      if (T) {
        HVar h = hoist(*T, g.expr[d], g.hv[d], a, laux);
        if (assign) {
          set_unknown(d + 1);
          g.expr[d + 1] = g.expr[d] + (laux ? "/k" : "/s") + std::to_string(a);
          g.hv[d + 1] = h;
          if (h.fam >= 0) g.csrc.at(d + 1).push_back({h.fam, h.j});
        }
        return h.idx;
      }
      if (assign) set_unknown(d + 1);
      IDX(d);
      return "lookup_op(N, " + C(d) + ", " + u32(a) + ", " + u32(laux) + ")";
    };
    const std::string ek = "ek" + s;
    const std::string kindof = "(" + ek + " & 15u)";
    // a fresh anyPattern alternative: no error, no anchor seen
    const std::string alt_reset =
        "  " + ek + " = 0u;" + (g.uses_anchor ? " areg" + s + " = 0ull; apres" + s + " = 0ull;" : "") + "\n";
    // the next element of the per-rule loop at level `lv`, while there is one: back to its body
    auto next_elem = [&](const std::string& lv, const std::string& cur, uint32_t body) {
      return "  if (li" + lv + s + " + 1u < ll" + lv + s + ") { li" + lv + s + "++; " + cur + " = ni(lf" + lv + s + " + li" + lv +
             s + "); " + jump(body) + " }\n";
    };

    // the column loop whose END at `pc` was just emitted: its element cell, its hoist region and
    // its body, into the stream the loop began in
    auto close_cloop = [&](uint32_t pc, const std::string& lv) {
      if (cloops.empty() || cloops.back().end_pc != pc) return;
      ColLoop& cl = cloops.back();
      const std::string& p = cl.T.prefix;
      const std::vector<std::string> join{p + "n.kt"};
      *cl.outer << L(cl.body_pc) << ":;\n  const uint32_t " << p << "e = " << p << "c + li" << lv << s << " * KVC_W" << cl.fam
                << ";\n  const Node " << p << "n = " << col_macro("LD", cl.fam, 0) << "(" << p << "e);\n"
                << cl.T.flush(B.kern.grouped, &join) << cl.body.str() << "  }\n";
      wcur = cl.outer;
      cloops.pop_back();
    };

    for (uint32_t pc = R.rb; pc < R.re; pc++) {
      const Inst& in = ps.prog[pc];
      const uint32_t op = in.op & 0xFF, d = (in.op >> 8) & 0xFF, aux = (in.op >> 16) & 0xFF;
      const std::string cd = C(d), cn = C(d + 1);
      const uint32_t lv = aux & 3;
      const std::string L_lv = std::to_string(lv);
      std::ostream& w = *wcur;
      // (the body label of a column loop goes ahead of its hoist region, below)
      if (cloops.empty() || cloops.back().body_pc != pc) w << L(pc) << ":;\n";
      switch (op) {
        case OP_MAPCHK:
          w << "  if (" << absent_or(d, "!= NT_MAP") << ") " << raise(E_TYPE_MAP, in.a, in.c) << "\n";
          break;
        case OP_ARRCHK:
          w << "  if (" << absent_or(d, "!= NT_ARR") << ") " << raise(E_TYPE_ARR, in.a, in.c) << "\n";
          break;
        case OP_AREG: {
          const std::string bit = "(1ull << " + std::to_string(aux & 63) + ")";
          w << "  areg" << s << " |= " << bit << "; if (" << lookup(d, in.a, aux, false) << " != ABSENT) apres" << s
            << " |= " << bit << ";\n";
          break;
        }
        case OP_KEY:
          w << "  " << cn << " = " << lookup(d, in.a, aux, true) << "; if (" << cn << " == ABSENT) " << jump(in.b) << "\n";
          break;
        case OP_KEYV:
          w << "  " << cn << " = " << lookup(d, in.a, aux, true) << ";\n";
          break;
        case OP_KEYGLOB:
          if (G) throw std::runtime_error("kvjit: KEYGLOB in a rule group");
          set_unknown(d + 1);
          IDX(d);
          w << "  { uint32_t nd_; if (!keyglob_op(P, B, N, " << cd << ", " << u32(in.op) << ", " << u32(in.a) << ", "
            << u32(in.c) << ", &nd_, &kn" << s << ")) " << jump(in.b) << " " << cn << " = nd_; }\n";
          break;
        case OP_SCOPE_END:
          if (G) break;  // groups carry no pending error (decided where raised)
          if (in.c == 0) w << "  if (" << kindof << ") " << ek << " |= " << u32(aux << 4) << ";\n";
          else w << "  if (" << kindof << ") { " << ek << " |= " << u32(aux << 4) << "; " << jump(in.c, true) << " }\n";
          break;
        case OP_POS_END:
          if (G) throw std::runtime_error("kvjit: POS_END in a rule group");
          w << "  if (" << kindof << ") { if (" << ek << " & " << u32(EF_COND << 4) << ") " << ek << " = 0u; else "
            << jump(in.c, true) << " }\n";
          break;
        case OP_NEG:
          w << "  if (" << lookup(d, in.a, aux, false) << " != ABSENT) " << raise(E_NEG, in.b, in.c) << "\n";
          break;
        case OP_STAR:
          w << "  if (" << absent_or(d + 1, "== NT_NULL") << ") " << raise(E_STAR, in.b, in.c) << "\n";
          break;
        case OP_LEAF: {
          // one bit of the leaf's table word (a group: one bit per member, consecutive): hoisted
          // leaves read the word gathered (and, for an array, replaced by the AND over its
          // elements) once per region (HoistTable::flush); others load it here
          const uint32_t slot = G ? g.gslot.at(pc) : slot_for(in.a);
          const uint32_t word = slot / 32;
          HoistTable* T = known(d) ? table_for(d) : nullptr;
          std::string wx;
          if (T) {
            const HVar& hvd = g.hv[d];
            const std::string hn = hvd.node;
            wx = hn + "_w" + std::to_string(word);
            col_mark(hvd.fam, hvd.j, CU_LEAF);
            if (T->have.insert(wx).second) T->add_word(HWord{wx, hvd, word});
          } else {
            IDX(d);
            wx = "kv_leaf_word(P, N, (" + cd + " != ABSENT ? N[" + cd + "] : Node{0u, 0u, 0u, 0u}), " + u32(word) + ")";
          }
          if (G) {
            const uint32_t mask = g.gn >= 32 ? 0xFFFFFFFFu : (1u << g.gn) - 1u;
            w << "  { const uint32_t f_ = " << al << " & ~((" << wx << " >> " << u32(slot % 32) << ") & " << hex32(mask)
              << ");\n    if (f_) { " << gfin("f_", E_VALUE, in.b, in.c) << " " << al << " &= ~f_; if (!" << al << ") "
              << gdone() << " } }\n";
          } else {
            w << "  if (!(((" << wx << " >> " << u32(slot % 32) << ") & 1u) != 0u)) " << raise(E_VALUE, in.b, in.c) << "\n";
          }
          break;
        }
        case OP_VLEAF:  // pattern variables: the resource's substituted value (kvvars.cpp)
          if (G) throw std::runtime_error("kvjit: VLEAF in a rule group");
          if (known(d)) w << "  { const Node vn_ = " << NODE(d, CU_WIDE | CU_B) << ";\n";
          else {
            IDX(d);
            w << "  { Node vn_{0u, 0u, 0u, 0u}; if (" << cd << " != ABSENT) vn_ = N[" << cd << "];\n";
          }
          dleaf_fn();
          w << "    if (!g_dleaf_0(B, N, B.dleaf[(size_t)" << u32(in.a) << " * n_res + r], vn_)) "
            << raise(E_VALUE, in.b, in.c) << " }\n";
          break;
        case OP_RAISE:
          w << "  " << raise(in.b, in.a, in.c) << "\n";
          break;
        case OP_EXISTCHK:
          w << "  if (" << absent_or(d, "!= NT_ARR") << ") " << raise(E_EXIST_RESTYPE, in.a, in.c) << "\n";
          break;
        case OP_LENCHK:
          w << "  if (" << NODE(d, CU_WIDE | CU_B) << ".b < " << u32(in.a) << ") " << raise(E_LEN, in.b, in.c) << "\n";
          break;
        case OP_INDEX:
          w << "  " << cn << " = ni(" << NODE(d, CU_WIDE) << ".a + " << u32(in.a) << ");\n";
          set_unknown(d + 1);
          break;
        case OP_LOOP_BEGIN:
          if (R.kind == 0 && lv == 0) {  // stage loop: hand over to the fused loop
            set_unknown(d + 1);
            w << "  { rs" << s << " = " << u32(in.a + 1) << " | ACT_; goto " << R.se << "; }\n";
            break;
          }
          [[fallthrough]];  // nested loop, per rule
        case OP_EXIST_BEGIN:
          if (G && op == OP_EXIST_BEGIN) throw std::runtime_error("kvjit: EXIST in a rule group");
          {
            // the array is a path column (a root path, or a path in an element of a root-path
            // array's family): its elements from the rows of its family
            uint32_t f = kNoCol;
            HoistTable* AT = opt.colloops && B.kern.colloops && known(d) ? table_for(d) : nullptr;
            if (AT && AT->fam >= 0 && g.hv[d].fam == AT->fam && g.hv[d].j != kNoCol)
              f = family((uint32_t)AT->fam, AT->fam == 0 ? g.expr[d] : g.expr[d].substr(AT->troot.size()));
            if (f != kNoCol) {
              const std::string an = NODE(d, CU_WIDE | CU_B);
              set_unknown(d + 1);
              cloops.emplace_back();
              ColLoop& cl = cloops.back();
              cl.body_pc = pc + 1;
              cl.end_pc = in.a;
              cl.fam = f;
              cl.troot = "P" + std::to_string(pc);
              cl.T.prefix = "p" + std::to_string(pc) + "_";
              cl.T.fam = (int)f;
              cl.T.troot = cl.troot;
              cl.T.cell0 = cl.T.prefix + "e";
              cl.outer = wcur;
              g.expr[d + 1] = cl.troot;
              g.hv[d + 1] = HVar{cn, cl.T.prefix + "n", (int)f, 0u};
              // (an array's cell carries the word offset of its element rows in c; the loop runs
              // on an array only, whatever the checks ahead of it)
              w << "  { uint32_t " << cl.T.prefix << "c;\n  { const Node an_ = " << an << "; lf" << L_lv << s << " = an_.a; ll" << L_lv
                << s << " = node_type(an_.kt) == NT_ARR ? an_.b : 0u; li" << L_lv << s << " = 0u; " << cl.T.prefix
                << "c = an_.c;\n    if (ll" << L_lv << s << " == 0u) ";
              if (op == OP_LOOP_BEGIN) w << jump(in.a + 1);
              else w << raise(E_EXIST_FAIL, in.b, in.c);
              w << "\n    " << cn << " = ni(an_.a); }\n";
              wcur = &cl.body;
              break;
            }
          }
          set_unknown(d + 1);
          w << "  { const Node an_ = " << NODE(d, CU_WIDE | CU_B) << "; lf" << L_lv << s << " = an_.a; ll" << L_lv << s << " = an_.b; li"
            << L_lv << s << " = 0u;\n    if (an_.b == 0u) ";
          if (op == OP_LOOP_BEGIN) w << jump(in.a + 1);
          else w << raise(E_EXIST_FAIL, in.b, in.c);
          w << "\n    " << cn << " = ni(an_.a); }\n";
          break;
        case OP_LOOP_END:
          if (!G)  // groups carry no pending error
            w << "  if (" << kindof << ") { if (" << ek << " & " << u32(EF_COND << 4) << ") " << ek << " = 0u; else "
              << jump(in.c, true) << " }\n";
          w << next_elem(L_lv, cn, in.a + 1);
          set_unknown(d + 1);
          close_cloop(pc, L_lv);
          break;
        case OP_EXIST_END:
          if (G) throw std::runtime_error("kvjit: EXIST in a rule group");
          w << "  if (!" << kindof << ") " << jump(pc + 1) << "\n  " << ek << " = 0u;\n"
            << next_elem(L_lv, cn, in.a + 1) << "  " << raise(E_EXIST_FAIL, in.b, in.c) << "\n";
          set_unknown(d + 1);
          close_cloop(pc, L_lv);
          break;
        case OP_ALT_BEGIN:
          if (G) throw std::runtime_error("kvjit: anyPattern in a rule group");
          w << alt_reset;
          break;
        case OP_ALT_END:
          if (G) throw std::runtime_error("kvjit: anyPattern in a rule group");
          w << "  if (" << kindof << " == 0u) " << finish("ST_PASS") << "\n  if (" << kindof << " == E_CPU) "
            << finish("ST_CPU") << "\n";
          if (in.b) w << "  " << finish("ST_FAIL") << "\n";
          else w << alt_reset;
          break;
        case OP_DONE:  // the MatchPattern epilogue as one select chain (no per-lane branches)
          if (R.kind != 0) throw std::runtime_error("kvjit: rule end inside a fused loop");
          if (G) {  // the members alive here passed (no error: the anchor-key check does not apply)
            w << "  { rs" << s << " = FIN_ | ST_PASS; goto " << R.se << "; }\n";
            break;
          }
          w << "  { const uint32_t k_ = " << kindof << ";\n    rs" << s << " = FIN_ | (k_ == 0u ? ST_PASS : k_ == E_CPU ? ST_CPU : ("
            << ek << " & " << u32((EF_COND | EF_GLOBAL) << 4) << ") ? ST_SKIP : ";
          if (g.uses_anchor) w << "(areg" << s << " & ~apres" << s << ") ? ST_ERROR : ";
          w << "k_ == E_LEN ? ST_ERROR : ST_FAIL);\n    goto " << R.se << "; }\n";
          break;
        default:  // OP_NOP, OP_METACHK (handled per resource by RF_BAD_META)
          break;
      }
    }
    if (!cloops.empty()) throw std::runtime_error("kvjit: a loop of rule " + std::to_string(g.ri) + " does not end in its region");
  }

  RGen analyze(uint32_t ri) {
    RGen g;
    g.ri = ri;
    g.s = "_" + std::to_string(ri);
    g.b = ps.rules[ri].prog;
    g.e = prog_end(ps, g.b);
    int nest = 0;
    for (uint32_t pc = g.b; pc <= g.e; pc++) {
      const Inst& in = ps.prog[pc];
      const uint32_t op = in.op & 0xFF, d = (in.op >> 8) & 0xFF, aux = (in.op >> 16) & 0xFF;
      g.maxd = std::max(g.maxd, d + 2);
      if (op == OP_AREG) g.uses_anchor = true;
      if (op == OP_KEYGLOB) g.uses_keyglob = true;
      if (op == OP_LOOP_BEGIN || op == OP_EXIST_BEGIN) {
        if (op == OP_LOOP_BEGIN && nest == 0 && (aux & 3) == 0) g.loops.push_back({pc, in.a});
        g.max_level = std::max(g.max_level, aux & 3);
        nest++;
      } else if (op == OP_LOOP_END || op == OP_EXIST_END) {
        nest--;
      }
    }
    g.expr.assign(g.maxd + 1, "");
    g.hv.assign(g.maxd + 1, HVar{});
    g.csrc.assign(g.maxd + 2, {});
    g.expr[0] = "R";
    g.hv[0] = HVar{"root", "rootn", 0, 0u};
    return g;
  }

  // The ops a lane runs after leaving stage loop k of `g` with a (non-condition) error,
  // from the LOOP_END's catch target: pure when it only carries the error through scope
  // ends to DONE (or to the end of the last anyPattern alternative), adding `flags`. The
  // rule's status is then a function of the error alone, decided at the failing element.
  struct PostChain {
    bool pure = false, alt = false;
    uint32_t flags = 0;
  };
  PostChain post_chain(const RGen& g, uint32_t pc, bool cond = false) const {
    PostChain r;
    for (int steps = 0; steps < 100000 && pc >= g.b && pc <= g.e; steps++) {
      const Inst& in = ps.prog[pc];
      const uint32_t op = in.op & 0xFF, aux = (in.op >> 16) & 0xFF;
      switch (op) {
        case OP_SCOPE_END:
          r.flags |= aux;
          cond |= (aux & EF_COND) != 0;
          pc = in.c ? in.c : pc + 1;
          continue;
        case OP_POS_END:
        case OP_LOOP_END:
          if (cond) return r;  // a condition error is cleared there: the walk goes on
          pc = in.c;
          continue;
        case OP_NOP:
        case OP_METACHK:
          pc++;
          continue;
        case OP_DONE:
          r.pure = true;
          return r;
        case OP_ALT_END:
          if (in.b) r.pure = r.alt = true;  // the last alternative: FAIL (or CPU)
          return r;
        default:
          return r;
      }
    }
    return r;
  }

  // Status of a rule whose error `ekx` reached DONE (or the last alternative's end): the
  // MatchPattern epilogue as one select chain
  std::string done_status(const RGen& g, const std::string& ekx, bool alt) const {
    std::ostringstream w;
    const std::string k = "(" + ekx + " & 15u)";
    if (alt) {
      w << "(" << k << " == 0u ? ST_PASS : " << k << " == E_CPU ? ST_CPU : ST_FAIL)";
      return w.str();
    }
    w << "(" << k << " == 0u ? ST_PASS : " << k << " == E_CPU ? ST_CPU : (" << ekx << " & "
      << u32((EF_COND | EF_GLOBAL) << 4) << ") ? ST_SKIP : ";
    if (g.uses_anchor) w << "(areg" << g.s << " & ~apres" << g.s << ") ? ST_ERROR : ";
    w << k << " == E_LEN ? ST_ERROR : ST_FAIL)";
    return w.str();
  }

  // Structural form of rule ri's program for rule groups: its ops with their operands, jump
  // targets relative to the program start; the pattern nodes and leaf predicates are left out
  // (listed in pns / preds, the LEAF pcs relative to the start in leafpcs). Empty when the
  // program holds an op a group cannot run: condition anchors (errors cleared later), existence
  // anchors, anyPattern, wildcard keys, pattern variables. Computed once per rule and image.
  const Form& form_of(uint32_t ri) {
    const auto [it, fresh] = forms.try_emplace(ri);
    if (fresh) group_form(ri, &it->second);
    return it->second;
  }
  void group_form(uint32_t ri, Form* F) const {
    const RuleRec& rr = ps.rules[ri];
    // (pattern-variable rules stay out of groups: their substitution status is decided per
    // member before the walk, and a group's record layout may be per resource slot)
    // (nor rules with preconditions: their gate is applied per rule before the walk)
    // (nor deny rules: they have no program)
    if (rr.route != 0 || rr.dyn || rr.pre || rr.deny) return;
    const uint32_t b = rr.prog, e = prog_end(ps, b);
    std::ostringstream f;
    auto rel = [&](uint32_t t) { return (int64_t)t - (int64_t)b; };
    for (uint32_t pc = b; pc <= e; pc++) {
      const Inst& in = ps.prog[pc];
      const uint32_t op = in.op & 0xFF, aux = (in.op >> 16) & 0xFF;
      f << (in.op & 0xFFFFFFu) << ':';  // op | depth << 8 | aux << 16
      switch (op) {
        case OP_MAPCHK:
        case OP_ARRCHK: F->pns.push_back(in.a); f << rel(in.c); break;
        case OP_AREG:
        case OP_KEYV:
        case OP_INDEX: f << in.a; break;
        case OP_KEY: f << in.a << ',' << rel(in.b); break;
        case OP_SCOPE_END:
          if (aux & EF_COND) return;
          f << (in.c ? rel(in.c) : -1);
          break;
        case OP_NEG: f << in.a << ','; F->pns.push_back(in.b); f << rel(in.c); break;
        case OP_STAR: F->pns.push_back(in.b); f << rel(in.c); break;
        case OP_LEAF:
          F->preds.push_back(in.a);
          F->leafpcs.push_back(pc - b);
          F->pns.push_back(in.b);
          f << rel(in.c);
          break;
        case OP_RAISE: f << in.b << ','; F->pns.push_back(in.a); f << rel(in.c); break;
        case OP_LENCHK: f << in.a << ','; F->pns.push_back(in.b); f << rel(in.c); break;
        case OP_LOOP_BEGIN: f << rel(in.a); break;
        case OP_LOOP_END: f << rel(in.a) << ',' << rel(in.c); break;
        case OP_DONE:
        case OP_NOP:
        case OP_METACHK: break;
        default: return;
      }
      f << ';';
    }
    F->text = f.str();
  }

  // A rule whose match reads the resource name is evaluated per resource behind its match bit
  // (which the tuple kernel sets to 1).
  bool name_dependent(uint32_t ri) const {
    const RuleRec& rr = ps.rules[ri];
    for (uint32_t f = rr.m_first; f < rr.m_first + rr.m_count; f++)
      if (ps.filters[f].flags & (MF_NAME | MF_NAMES)) return true;
    for (uint32_t f = rr.x_first; f < rr.x_first + rr.x_count; f++)
      if (ps.filters[f].flags & (MF_NAME | MF_NAMES)) return true;
    return false;
  }
  // the match of rule ri at LDS row `row` of kernel `kn`: its bit of the kernel's match words
  std::string mt_cond(const Kern& kn, uint32_t ri, uint32_t row) const {
    const uint32_t p = kn.mt_kbase * 32u + row;
    std::string c = "((mw" + std::to_string(p / 32u) + " >> " + std::to_string(p % 32u) + "u) & 1u)";
    if (name_dependent(ri)) c += " && g_match_" + std::to_string(ri) + "(P, B, R, rkind, rflags)";
    return c;
  }

  // ================================================================ one fused block
  // The code of one fused block inside a kernel body (its own C++ scope), in passes over a Block
  // (fused_block, at the end, runs them): form_groups, prepare_rules, per stage emit_segment and
  // emit_fused_loops, emit_rule_state; all over the status and record emitters.
  //
  // Lean rules: at the end of stage segment k a rule that enters stage loop k keeps only one bit
  // (am<k>_<w>, bit q of its block position), one that jumps past the loop one bit of sk<k>_<w>
  // (its single target), and one that finished stores its status at once; inside the fused loop
  // its error state is local to the element and an element that fails decides the status there
  // (post_chain), so no per-rule register lives across the loop. After the loops the resume pc is
  // rebuilt from the bits.

  void form_groups(const std::vector<uint32_t>& rules_in, Block* B) {
    std::map<std::string, size_t> open;  // form -> the group that still takes members
    for (uint32_t ri : rules_in) {
      const Form& F = form_of(ri);
      if (F.text.empty()) continue;
      auto it = open.find(F.text);
      if (it != open.end()) {
        GInfo& G = B->ginfo[it->second];
        const uint32_t dp = F.pns.empty() ? 0u : F.pns[0] - G.pns0[0];
        bool ok = G.members.size() < 32;
        for (size_t i = 0; i < F.pns.size() && ok; i++) ok = F.pns[i] - G.pns0[i] == dp;
        if (ok) {
          G.members.push_back(ri);
          G.dpn.push_back(dp);
          G.preds.push_back(F.preds);
          B->gof[ri] = it->second;
          continue;
        }
      }
      GInfo G;
      G.members = {ri};
      G.pns0 = F.pns;
      G.leafpcs = F.leafpcs;
      G.dpn = {0u};
      G.preds = {F.preds};
      open[F.text] = B->ginfo.size();
      B->gof[ri] = B->ginfo.size();
      B->ginfo.push_back(std::move(G));
    }
    // block order: a group's members together, at its first member's place
    for (uint32_t ri : rules_in) {
      bool member;
      const GInfo* G = B->group_of(ri, &member);
      if (!G) B->rules.push_back(ri);
      else if (!member) B->rules.insert(B->rules.end(), G->members.begin(), G->members.end());
    }
  }

  // The group state of representative `g` (at block position g->q): its site descriptor, its
  // members' record layout, their leaf predicates and slots, its member table. Every id here
  // (kern.gsn, gs_members, the memo slots, gtab_n) is handed out in call order.
  void prepare_group(const GInfo& G, Block* B, RGen* gp) {
    RGen& g = *gp;
    Kern& kern = B->kern;
    g.grp = true;
    g.s = "_G" + std::to_string(B->hbase + g.q);
    g.gn = (uint32_t)G.members.size();
    g.gri = G.members;
    g.gdpn = G.dpn;
    if (g.gn >= 2u) {
      g.gsite = true;
      g.gl = kern.gsn++;
      g.gpre = gs_members;
      gs_desc.insert(gs_desc.end(), {g.gn, gs_members, (uint32_t)(gs_mem.size() / 2u), 0u});
      for (uint32_t j = 0; j < g.gn; j++) gs_mem.insert(gs_mem.end(), {G.members[j], G.dpn[j]});
      gs_members += g.gn;
    }
    // (site-record members get their records expanded to their resource slots at fetch)
    if (g.gsite || g.gn >= kGslotMembers)
      for (uint32_t m : G.members) rec_slot.at(m) = 1;
    g.grow = B->hbase + g.q;
    for (const auto& m : G.preds)
      for (uint32_t pi : m) pred_fn(pi);
    for (size_t i = 0; i < G.leafpcs.size(); i++) {
      std::vector<uint32_t> lp;
      for (const auto& m : G.preds) lp.push_back(m[i]);
      g.gslot[g.b + G.leafpcs[i]] = group_slots(lp);
    }
    // members as arithmetic progressions (rule ids, node shifts), else a table
    bool arith = true;
    g.gsri = g.gn > 1 ? g.gri[1] - g.gri[0] : 0u;
    g.gspn = g.gn > 1 ? g.gdpn[1] : 0u;
    for (uint32_t j = 0; j < g.gn && arith; j++) arith = g.gri[j] == g.gri[0] + j * g.gsri && g.gdpn[j] == j * g.gspn;
    if (!arith) {
      g.gtab = "kvg_t" + std::to_string(gtab_n++);
      std::ostringstream t;
      t << "__device__ const uint32_t " << g.gtab << "[" << 2 * g.gn << "] = {";
      for (uint32_t j = 0; j < g.gn; j++) t << u32(g.gri[j]) << ", ";
      for (uint32_t j = 0; j < g.gn; j++) t << u32(g.gdpn[j]) << (j + 1 < g.gn ? ", " : "");
      t << "};\n";
      kern.decls += t.str();
    }
  }

  void prepare_rules(Block* B) {
    for (uint32_t q = 0; q < B->rules.size(); q++) {
      const uint32_t ri = B->rules[q];
      if (no_program(ps.rules[ri])) continue;
      bool member;
      const GInfo* G = B->group_of(ri, &member);
      if (member) continue;  // runs as one bit of its group's representative
      RGen g = analyze(ri);
      g.q = q;
      for (uint32_t pc = g.b; pc <= g.e; pc++)
        if ((ps.prog[pc].op & 0xFF) == OP_LEAF) pred_fn(ps.prog[pc].a);
      if (G) prepare_group(*G, B, &g);
      B->K = std::max(B->K, g.loops.size());
      g.lean.assign(g.loops.size(), 0);
      g.post_flags.assign(g.loops.size(), 0);
      g.post_alt.assign(g.loops.size(), 0);
      g.skip_to.assign(g.loops.size(), 0xFFFFFFFFu);
      B->gs.push_back(std::move(g));
    }
  }

  // ---------------------------------------------------------------- status and record emitters
  // word / bit of block position q in the stage-k masks `m` ("am": active in the loop, "sk":
  // jumped past it)
  static std::string mword(const char* m, size_t k, uint32_t q) {
    return std::string(m) + std::to_string(k) + "_" + std::to_string(q / 32);
  }
  static std::string mbit(uint32_t q) { return u32(1u << (q % 32)); }
  // status row of block position q: its LDS address and row index
  static std::string row(const Block& B, uint32_t q) {
    return "s_w + " + u32(KV_ROW0 + (B.hbase + q) * KV_RSTRIDE) + ", " + u32(B.hbase + q);
  }
  // "no error pending" in rule g's registers
  static std::string clear_err(const RGen& g) {
    std::string c = "ek" + g.s + " = 0u;";
    for (uint32_t lv = 0; lv <= g.max_level && lv < 4; lv++) c += " ei" + std::to_string(lv) + g.s + " = 0u;";
    if (g.uses_keyglob) c += " ekn" + g.s + " = ABSENT;";
    return c;
  }
  // EState of rule g from its registers (error kind / flags / pattern node in `ekx`)
  static std::string estate(const RGen* g, const std::string& ekx) {
    if (!g) return "EState e_{0u, 0u, 0u, ABSENT, ABSENT, 0u, 0u, 0u, 0u};";
    std::ostringstream k;
    k << "EState e_{" << ekx << " & 15u, (" << ekx << " >> 4) & 15u, " << ekx << " >> 8, "
      << (g->uses_keyglob ? "ekn" + g->s : std::string("ABSENT")) << ", ABSENT";
    for (uint32_t lv = 0; lv < 4; lv++) k << ", " << (lv <= g->max_level ? "ei" + std::to_string(lv) + g->s : "0u");
    k << "};";
    return k.str();
  }
  // status `st` + error record of the rule at block position q: its LDS status byte (copied to the
  // status matrix when the kernel ends) and the record (kv_final)
  std::string store_st(const Block& B, uint32_t q, const RGen* g, const std::string& st, const std::string& ekx) const {
    std::ostringstream k;
    k << "  { " << estate(g, ekx) << "\n    kv_final(O, " << B.rules[q] << "u, n_res, r, valid, " << st << ", e_, "
      << row(B, q) << "); }\n";
    return k.str();
  }
  // the final status in rs of the rule at block position q, unless it was stored already or is
  // NOMATCH (the rows' prefill)
  std::string store(const Block& B, uint32_t q) const {
    const RGen* g = B.at(q);
    const std::string s = g ? g->s : "_" + std::to_string(B.rules[q]);
    const std::string st = "rs" + s + " & 0xFFu";
    if (!g) return store_st(B, q, g, st, "0u");
    // the members alive at a group's end passed: their PASS was staged by the match code
    // (a group ends only at DONE, ST_PASS, or with every member decided, ST_STORED_)
    if (g->grp) return std::string();
    return "  if ((rs" + s + " & 0xFFu) != ST_STORED_ && (rs" + s + " & 0xFFu) != ST_NOMATCH) {\n" +
           store_st(B, q, g, st, "ek" + s) + "  }\n";
  }
  // match / route of the rule at block position q (rs = its first pc, or FIN | status); of a
  // group: every member's, the matched ones alive (al), the others stored
  std::string match_code(const Block& B, uint32_t q) const {
    const RGen* g = B.at(q);
    return g && g->grp ? group_match_code(B, *g) : rule_match_code(B, q);
  }
  std::string group_match_code(const Block& B, const RGen& g) const {
    // a group's members are consecutive rows, so their match bits are consecutive bits of the
    // block's match words: one extract instead of a branch per member. Statuses are staged
    // here, branch-free: PASS for every member that runs (a failure overwrites its byte where
    // it is raised, so the group's end stores nothing), CPU for the members an anchor-error
    // phrase or a panicking labels / annotations shape routes (rows start as NOMATCH; 0xFF
    // past the batch)
    std::ostringstream k;
    const uint32_t p0 = B.kern.mt_kbase * 32u + g.grow, w0 = p0 / 32u, s0 = p0 % 32u;
    const uint32_t mask = g.gn >= 32 ? 0xFFFFFFFFu : (1u << g.gn) - 1u;
    k << "  { uint32_t mt_ = ((mw" << w0 << " >> " << s0 << "u)";
    if (s0 + g.gn > 32u) k << " | (mw" << (w0 + 1) << " << " << (32u - s0) << "u)";
    k << ") & " << hex32(mask) << ";\n";
    for (uint32_t j = 0; j < g.gn; j++)
      if (name_dependent(g.gri[j]))
        k << "    if (((mt_ >> " << j << "u) & 1u) && !g_match_" << g.gri[j] << "(P, B, R, rkind, rflags)) mt_ &= "
          << hex32(~(1u << j)) << ";\n";
    k << "    uint32_t cpu_ = (rflags & RF_MAGIC) ? mt_ : 0u;\n";
    for (uint32_t j = 0; j < g.gn; j++) {
      const RuleRec& rr = ps.rules[g.gri[j]];
      if (rr.flags & RR_META_EXPAND)
        k << "    cpu_ |= (rflags & " << u32(meta_bad_flags(rr.flags)) << ") ? (mt_ & " << u32(1u << j) << ") : 0u;\n";
    }
    for (uint32_t j = 0; j < g.gn; j++)
      k << "    s_w[" << u32(KV_ROW0 + (g.grow + j) * KV_RSTRIDE) << " + threadIdx.x] = valid ? (uint8_t)(((mt_ >> " << j
        << "u) & 1u) ? (((cpu_ >> " << j << "u) & 1u) ? ST_CPU : ST_PASS) : ST_NOMATCH) : (uint8_t)0xFFu;\n";
    k << "    al" << g.s << " = mt_ & ~cpu_; }\n";
    k << "  rs" << g.s << " = al" << g.s << " ? " << u32(g.b) << " : FIN_ | ST_STORED_;\n";
    return k.str();
  }
  std::string rule_match_code(const Block& B, uint32_t q) const {
    const uint32_t ri = B.rules[q];
    const RuleRec& rr = ps.rules[ri];
    const std::string s = "_" + std::to_string(ri);
    std::ostringstream k;
    k << "  if (" << mt_cond(B.kern, ri, B.hbase + q) << ") {\n";
    switch (rr.route) {
      case 1: k << "    rs" << s << " = FIN_ | ST_CPU;\n"; break;
      case 2: k << "    rs" << s << " = FIN_ | ST_NOMATCH;\n"; break;
      case 3: k << "    rs" << s << " = FIN_ | " << u32(rr.const_status) << ";\n"; break;
      default:
        k << "    if (rflags & RF_MAGIC) rs" << s << " = FIN_ | ST_CPU;\n";
        if (rr.flags & RR_META_EXPAND)
          k << "    else if (rflags & " << u32(meta_bad_flags(rr.flags)) << ") rs" << s << " = FIN_ | ST_CPU;\n";
        if (rr.pre)  // preconditions precede pattern substitution (validation.go:175-193)
          k << "    else if (B.pre_st[(size_t)" << (rr.pre - 1) << "u * n_res + r]) rs" << s << " = FIN_ | B.pre_st[(size_t)"
            << (rr.pre - 1) << "u * n_res + r];\n";
        if (rr.dyn)
          k << "    else if (B.dyn_st[(size_t)" << (rr.dyn - 1) << "u * n_res + r]) rs" << s << " = FIN_ | B.dyn_st[(size_t)"
            << (rr.dyn - 1) << "u * n_res + r];\n";
        if (rr.deny)  // validate.deny (validation.go:195-197): the fold's plane is the status
          k << "    else rs" << s << " = FIN_ | B.deny_st[(size_t)" << (rr.deny - 1) << "u * n_res + r];\n";
        else
          k << "    else rs" << s << " = " << u32(rr.prog) << ";\n";
        break;
    }
    k << "  }\n";
    return k.str();
  }

  // ---------------------------------------------------------------- stage segments
  // ops [first, end) of rule g's stage-k segment: from the start (or the end of stage loop k - 1)
  // to the LOOP_BEGIN of stage loop k (included), or to DONE
  static std::pair<uint32_t, uint32_t> segment(const RGen& g, size_t k) {
    return {k == 0 ? g.b : g.loops[k - 1].second + 1, k < g.loops.size() ? g.loops[k].first + 1 : g.e + 1};
  }

  // Is rule g lean in stage loop k? Decided when its stage-k segment has been emitted, from the
  // targets past the segment that it jumps to without / with a pending error. Lean when the post
  // chain of the loop is pure and the segment leaves at most one way past the loop, whose chain is
  // pure for any pending error (a lane that jumps there with an error is decided at once; one
  // without resumes there after the loop).
  struct LeanDecision {
    bool lean = false;
    bool alt = false;                                  // the error chains end at the last anyPattern alternative
    PostChain post;                                    // chain of the loop's own catch target
    std::set<uint32_t> okset;                          // every way past the loop without an error
    std::vector<std::pair<uint32_t, PostChain>> errc;  // ... with one: target and its chain
    std::set<uint32_t> carry_ok, carry_err;            // RGen::carry_ok / carry_err after this stage
  };
  LeanDecision lean_decision(const RGen& g, size_t k, const std::set<uint32_t>& jumps,
                             const std::set<uint32_t>& err_jumps) const {
    LeanDecision D;
    const uint32_t se = segment(g, k).second, le = g.loops[k].second;
    D.post = post_chain(g, ps.prog[le].c);
    // every way past loop k: this segment's jumps and the targets of earlier stages that lie
    // beyond this segment (they pass through it)
    D.okset = jumps;
    std::set<uint32_t> errset = err_jumps;
    for (uint32_t t : g.carry_ok)
      if (t >= se) D.okset.insert(t);
    for (uint32_t t : g.carry_err)
      if (t >= se) errset.insert(t);
    D.lean = D.post.pure && D.okset.size() <= 1;
    for (uint32_t t : errset) {
      D.errc.push_back({t, post_chain(g, t, true)});
      D.lean &= D.errc.back().second.pure;
    }
    D.alt = !D.errc.empty() && D.errc[0].second.alt;
    for (auto& e : D.errc) D.lean &= e.second.alt == D.alt;
    D.carry_ok = D.okset;
    if (!D.lean) {  // (a lean rule's errors past the loop are decided at the segment end)
      D.carry_ok.insert(le + 1);
      D.carry_err = errset;
      D.carry_err.insert(ps.prog[le].c);
    }
    return D;
  }

  // the end of a lean rule's stage-k segment: its bit of the stage masks, or its status at once
  void lean_exit(const Block& B, RGen& g, size_t k, const LeanDecision& D, std::ostream& seg) const {
    const std::string ek = "ek" + g.s;
    seg << "  if (rs" << g.s << " & ACT_) " << mword("am", k, g.q) << " |= " << mbit(g.q) << ";\n";
    if (!D.okset.empty() || !D.errc.empty()) {
      // past the loop: with an error the status is decided now, else resume there later
      seg << "  else if (rs" << g.s << " < FIN_) {\n";
      if (!D.errc.empty()) {
        std::string fl = "0u";
        for (auto it = D.errc.rbegin(); it != D.errc.rend(); ++it)
          fl = "(rs" + g.s + " == " + u32(it->first) + " ? " + u32(it->second.flags << 4) + " : " + fl + ")";
        const std::string ekx = "(" + ek + " | " + fl + ")";
        seg << "    if (" << ek << " & 15u) {\n" << store_st(B, g.q, &g, done_status(g, ekx, D.alt), ekx) << "    }\n";
      }
      if (!D.okset.empty()) {
        g.skip_to[k] = *D.okset.begin();
        seg << "    " << (D.errc.empty() ? "" : "else ") << mword("sk", k, g.q) << " |= " << mbit(g.q) << ";\n";
      }
      seg << "  }\n";
    }
    seg << "  else {\n" << store(B, g.q) << "  }\n";
  }

  // rule g's stage-k segment: (stage 0) its match code, (after a lean loop) its resume pc from
  // the mask bits, the dispatch on rs, the ops; then its status when the rule ends here, else the
  // lean decision for stage loop k and a lean rule's exit
  void emit_segment(Block& B, RGen& g, size_t k, std::ostream& seg) {
    const auto [sb, se] = segment(g, k);
    Region R;
    R.kind = 0;
    R.rb = sb;
    R.re = se;
    R.jre = se;
    R.se = "R" + std::to_string(g.ri) + "_S" + std::to_string(k);
    std::set<uint32_t> jumps, err_jumps;
    R.jumps = &jumps;
    R.err_jumps = &err_jumps;
    std::ostringstream w;
    emit_region(B, g, R, w);
    if (k == 0) seg << match_code(B, g.q);  // just before its first segment: rs is born here
    if (k > 0 && g.lean[k - 1]) {  // resume pc of a lean rule from its stage-(k-1) bits
      const uint32_t le = g.loops[k - 1].second;
      seg << "  rs" << g.s << " = (" << mword("am", k - 1, g.q) << " & " << mbit(g.q) << ") ? " << u32(le + 1) << " : ";
      if (g.skip_to[k - 1] != 0xFFFFFFFFu)
        seg << "(" << mword("sk", k - 1, g.q) << " & " << mbit(g.q) << ") ? " << u32(g.skip_to[k - 1]) << " : ";
      seg << "FIN_ | ST_STORED_;\n";
      // the error state of a lane that left the loop clean (no register of the rule lives
      // across the loop)
      seg << "  " << clear_err(g) << "\n";
    }
    seg << "  // rule " << g.ri << " stage " << k << "\n  switch (rs" << g.s << ") {\n";
    if (k == 0) seg << "    case " << u32(g.b) << ": goto R" << g.ri << "_L" << g.b << ";\n";
    for (uint32_t t : g.resume)
      if (t >= sb && t < se) seg << "    case " << u32(t) << ": goto R" << g.ri << "_L" << t << ";\n";
    seg << "    default: goto " << R.se << ";\n  }\n" << w.str() << R.se << ":;\n";
    if (k == g.loops.size()) {
      seg << store(B, g.q);  // the rule has finished for every lane
      return;
    }
    const LeanDecision D = lean_decision(g, k, jumps, err_jumps);
    g.carry_ok = D.carry_ok;
    g.carry_err = D.carry_err;
    g.lean[k] = D.lean;
    g.post_flags[k] = D.post.flags;
    g.post_alt[k] = D.post.alt;
    if (D.lean) lean_exit(B, g, k, D, seg);
  }

  // ---------------------------------------------------------------- fused loops
  // One fused loop of stage k: the array its rules walk, the element's names (el / eln / ec / fli
  // + tag) and the hoist table of the lookups from the element
  struct Loop {
    size_t k = 0;
    std::string tag, troot;
    uint32_t fam = kNoCol;  // the family of the array's elements (kNoCol: walk the node rows)
    HoistTable T;
  };

  // Rule g's body of stage loop k inside fused loop L. Every form tests whether the rule is active
  // in the loop, points its cursor at the element, runs the region and lands on the LOOP_END's
  // label; the ending differs: a group stops when no member is left; a lean rule's error is local
  // to the element and one that leaves the loop decides the status now; a plain rule carries its
  // error out of the loop in rs.
  void loop_body(Block& B, RGen& g, Loop& L, std::ostream& out) {
    const size_t k = L.k;
    const uint32_t lb = g.loops[k].first, le = g.loops[k].second;
    const uint32_t d = (ps.prog[lb].op >> 8) & 0xFF;
    g.expr[d + 1] = L.troot;
    g.hv[d + 1] = HVar{"el" + L.tag, "eln" + L.tag, L.fam != kNoCol ? (int)L.fam : -1, L.fam != kNoCol ? 0u : kNoCol};
    Region R;
    R.kind = 1;
    R.rb = lb + 1;
    R.re = le;  // LOOP_END emitted below
    R.jre = le + 1;
    R.li0 = "fli" + L.tag;
    R.T = &L.T;
    R.troot = L.troot;
    std::ostringstream w;
    emit_region(B, g, R, w);
    const Inst& end = ps.prog[le];
    if (end.c <= le) throw std::runtime_error("kvjit: loop exit target inside the loop");
    const bool lean = g.lean[k];
    const std::string ek = "ek" + g.s, rs = "rs" + g.s, am = mword("am", k, g.q), bit = mbit(g.q);
    out << "    if (" << (lean ? am + " & " + bit : rs + " & ACT_") << ") {\n";
    if (lean && !g.grp) out << "      " << clear_err(g) << "\n";  // element-local error state
    out << "      c" << (d + 1) << g.s << " = el" << L.tag << ";\n" << w.str() << "R" << g.ri << "_L" << le << ":;\n";
    if (g.grp) {  // errors were decided where raised: a group with no member left stops
      out << "      if (!al" << g.s << ") " << (lean ? am + " &= ~" + bit : rs + " = FIN_ | ST_STORED_") << ";\n";
    } else {
      out << "      if (" << ek << " & 15u) { if (" << ek << " & " << u32(EF_COND << 4) << ") " << ek << " = 0u; else ";
      if (lean) {  // an error that leaves the loop decides the status now
        const std::string ekx = g.post_flags[k] ? "(" + ek + " | " + u32(g.post_flags[k] << 4) + ")" : ek;
        out << "{\n        " << am << " &= ~" << bit << ";\n"
            << "  " << store_st(B, g.q, &g, done_status(g, ekx, g.post_alt[k]), ekx) << "      } }\n";
      } else {
        out << rs << " = " << u32(end.c) << "; }\n";
        g.resume.insert(end.c);
      }
    }
    out << "    }\n";
    g.resume.insert(le + 1);
    for (uint32_t x = d + 1; x < g.expr.size(); x++) g.expr[x].clear();  // loop-local exprs end here
  }

  // the fused loop `tag` of stage k over the array at symbolic cursor `key` ("U<ri>": unknown,
  // one rule's own), walked once for the rules `grp`
  void emit_fused_loop(Block& B, size_t k, const std::string& key, const std::vector<RGen*>& grp, const std::string& tag,
                       std::ostream& body) {
    const RGen& g0 = *grp[0];
    const uint32_t d0 = (ps.prog[g0.loops[k].first].op >> 8) & 0xFF;
    const std::string arr_node = key[0] == 'U' ? "N[c" + std::to_string(d0) + g0.s + "]" : g0.hv[d0].node;
    if (key[0] == 'U') {
      for (const auto& cj : g0.csrc.at(d0)) col_mark(cj.first, cj.second, CU_WIDE);
    } else {
      col_mark(g0.hv[d0].fam, g0.hv[d0].j, CU_WIDE | CU_B);  // an_.a / .b / .c below
    }
    Loop L;
    L.k = k;
    L.tag = tag;
    L.troot = "E" + tag;
    L.T.prefix = "l" + tag + "_";
    // the elements' lookups from the columns of the array's family (the array must be a
    // column itself: its cell carries the offset of its element rows)
    L.fam = key[0] == 'R' && fams[0].idx.count(key) ? family(key) : kNoCol;
    if (L.fam != kNoCol) {
      L.T.fam = (int)L.fam;
      L.T.troot = L.troot;
      L.T.cell0 = "ec" + tag;
    }
    std::ostringstream bodies;
    for (RGen* gp : grp) loop_body(B, *gp, L, bodies);
    std::vector<uint32_t> gmask(B.mask_words(), 0);  // lean rules of the loop, per mask word
    for (const RGen* gp : grp)
      if (gp->lean[k]) gmask[gp->q / 32] |= 1u << (gp->q % 32);
    body << "  { // fused loop " << tag << " over " << key << " (" << grp.size() << " rules)\n"
         << "    uint32_t fn" << tag << " = 0u, ff" << tag << " = 0u, fe" << tag << " = 0u;\n    if (((0u";
    for (const RGen* gp : grp)
      if (!gp->lean[k]) body << " | rs" << gp->s;
    body << ") & ACT_)";
    for (uint32_t w = 0; w < gmask.size(); w++)
      if (gmask[w]) body << " | (am" << k << "_" << w << " & " << u32(gmask[w]) << ")";
    body << ") { const Node an_ = " << arr_node << "; ff" << tag << " = an_.a; fn" << tag << " = an_.b; fe" << tag
         << " = an_.c; }\n";
    body << "    for (uint32_t fli" << tag << " = 0u; fli" << tag << " < fn" << tag << "; fli" << tag << "++) {\n"
         << "      const uint32_t el" << tag << " = ni(ff" << tag << " + fli" << tag << ");\n";
    if (L.fam != kNoCol)  // the element's column-0 cell: element row fe + i of its family
      body << "      const uint32_t ec" << tag << " = fe" << tag << " + fli" << tag << " * KVC_W" << L.fam
           << ";\n      const Node eln" << tag << " = " << col_macro("LD", L.fam, 0) << "(ec" << tag << ");\n";
    else
      body << "      const Node eln" << tag << " = N[el" << tag << "];\n";
    body << L.T.flush(B.kern.grouped) << bodies.str() << "    }\n";
    for (const RGen* gp : grp)
      if (!gp->lean[k]) body << "    rs" << gp->s << " &= ~ACT_;\n";
    body << "  }\n";
  }

  // fused loops of stage k: the rules grouped by the symbolic cursor of the array their k-th
  // stage loop walks, in order of first use
  void emit_fused_loops(Block& B, size_t k, std::ostream& body) {
    std::map<std::string, std::vector<RGen*>> groups;
    std::vector<std::string> order;
    for (RGen& g : B.gs) {
      if (k >= g.loops.size()) continue;
      const uint32_t d = (ps.prog[g.loops[k].first].op >> 8) & 0xFF;
      const std::string key = g.expr[d].empty() ? "U" + std::to_string(g.ri) : g.expr[d];
      if (!groups.count(key)) order.push_back(key);
      groups[key].push_back(&g);
    }
    uint32_t li = 0;
    for (const std::string& key : order) emit_fused_loop(B, k, key, groups[key], std::to_string(k) + "_" + std::to_string(li++), body);
  }

  // per-rule state (rules of other routes only carry rs = FIN | status); a group's: rs and the
  // alive members
  void emit_rule_state(const Block& B, std::ostream& k) const {
    for (uint32_t ri : B.rules)
      if (!B.gof.count(ri)) k << "  uint32_t rs_" << ri << " = FIN_ | ST_NOMATCH;\n";
    for (const RGen& g : B.gs) {
      const std::string& s = g.s;
      if (g.grp) k << "  uint32_t rs" << s << " = FIN_ | ST_STORED_, al" << s << " = 0u;\n";
      k << "  uint32_t ek" << s << " = 0u";
      for (uint32_t lv = 0; lv <= g.max_level && lv < 4; lv++) k << ", ei" << lv << s << " = 0u";
      if (g.uses_keyglob) k << ", kn" << s << " = ABSENT, ekn" << s << " = ABSENT";
      k << ";\n";
      if (g.uses_anchor) k << "  uint64_t areg" << s << " = 0ull, apres" << s << " = 0ull;\n";
      k << "  uint32_t c0" << s << " = root";
      for (uint32_t d = 1; d < g.maxd; d++) k << ", c" << d << s << " = ABSENT";
      k << ";\n";
      k << "  uint32_t";
      for (uint32_t l = 0; l <= g.max_level && l < 4; l++)
        k << (l ? "," : "") << " li" << l << s << " = 0u, lf" << l << s << " = 0u, ll" << l << s << " = 0u";
      k << ";\n";
    }
  }

  // every resume pc must lie in a segment (else the rule would never finish)
  static void check_resumes(const Block& B) {
    for (const RGen& g : B.gs)
      for (uint32_t t : g.resume) {
        bool ok = false;
        for (size_t k = 0; k <= g.loops.size() && !ok; k++) ok = t >= segment(g, k).first && t < segment(g, k).second;
        if (!ok) throw std::runtime_error("kvjit: resume target " + std::to_string(t) + " of rule " +
                                         std::to_string(g.ri) + " is not in a segment");
      }
  }

  // The code of the fused block of `rules_in` in kernel `kern`, whose status rows start at row
  // `hbase` of the kernel; `order` receives the block's rules in block position order.
  std::string fused_block(Kern& kern, const std::vector<uint32_t>& rules_in, uint32_t hbase, std::vector<uint32_t>* order) {
    Block B(kern, hbase);
    form_groups(rules_in, &B);
    *order = B.rules;
    prepare_rules(&B);
    std::ostringstream body;  // everything after the per-rule declarations
    for (size_t k = 0; k <= B.K; k++) {
      std::ostringstream seg;  // the stage-k segments of every rule
      for (RGen& g : B.gs)
        if (k <= g.loops.size()) emit_segment(B, g, k, seg);
      if (k < B.K) {  // stage-k masks of the lean rules
        body << "  uint32_t";
        for (uint32_t w = 0; w < B.mask_words(); w++)
          body << (w ? "," : "") << " am" << k << "_" << w << " = 0u, sk" << k << "_" << w << " = 0u";
        body << ";\n";
      }
      body << B.global.flush(B.kern.grouped) << seg.str();  // (the segments' hoisted lookups ahead of them)
      if (k < B.K) emit_fused_loops(B, k, body);
    }
    check_resumes(B);
    std::ostringstream k;
    emit_rule_state(B, k);
    // rules of other routes are final after match / route
    for (uint32_t q = 0; q < B.rules.size(); q++)
      if (no_program(ps.rules[B.rules[q]])) k << match_code(B, q) << store(B, q);
    k << body.str();
    return k.str();
  }

  // One kernel running the fused chunks `chs` one after the other for each
  // resource: a workgroup re-reads its resources' node rows per chunk while they
  // are still cache-resident, instead of one grid-wide pass per chunk.
  // Statuses: one LDS row per rule of the kernel (KV_RSTRIDE bytes: a status byte per lane)
  // after the waves' record counters (KV_ROW0 bytes: a byte per (wave, rule)), prefilled with NOMATCH, flushed once when the kernel ends
  // (kv_end_flush: status matrix, per-rule and per-scope histograms). A per-block flush of
  // wave-private rows (round 4, first build) freed the LDS but cost C5 25 flushes per wave:
  // 3.91 against 3.25 ms per pass.
  static uint32_t kernel_lds(uint32_t nr) { return KV_ROW0 + nr * KV_RSTRIDE; }
  // waves per SIMD a CU's 160 KB LDS admits (workgroups of KV_RWAVES waves): allocations are made
  // in 1280 B granules (C3's 124-rule kernels, 32 240 B, ran at 4 workgroups of 4 waves per CU and
  // 1.3x the time of the 123-rule ones at 31 980 B; round 4, gpurun_out/r4h)
  static int lds_waves(uint32_t nr) {
    const uint32_t g = 1280u, b = (kernel_lds(nr) + g - 1u) / g * g;
    return (int)std::max<uint32_t>(1u, (160u * 1024u) / std::max(b, g) * KV_RWAVES / 4u);
  }
  // The kernel `name` of the blocks `chs` (each one's rules) at a bound of `waves` per SIMD
  // (0: none); returns its rules in LDS-row order (blocks reorder rule-group members).
  std::vector<uint32_t> group_kernel(const std::string& name, const std::vector<std::vector<uint32_t>>& chs, int waves,
                                     bool grouped, bool colloops) {
    std::vector<std::string> blocks;
    std::vector<std::pair<uint32_t, uint32_t>> rows;  // LDS rows [first, first + count) of each block
    std::vector<uint32_t> rules;
    uint32_t nr_all = 0;
    for (const auto& c : chs) nr_all += (uint32_t)c.size();
    // (the waves' record counters hold a byte per (wave, row): KV_KROWS rows)
    if (nr_all > KV_KROWS) throw std::runtime_error("kvjit: at most KV_KROWS rules per kernel (KVGPU_JIT_CHUNK)");
    Kern kern;
    kern.mt_kbase = (uint32_t)(mt_bits.size() / 32u);
    kern.gs0 = (uint32_t)(gs_desc.size() / 4u);
    kern.grouped = grouped;
    kern.colloops = colloops;
    for (const auto& c : chs) {
      std::vector<uint32_t> ord;
      rows.push_back({(uint32_t)rules.size(), (uint32_t)c.size()});
      blocks.push_back(fused_block(kern, c, (uint32_t)rules.size(), &ord));
      rules.insert(rules.end(), ord.begin(), ord.end());
    }
    mt_bits.insert(mt_bits.end(), rules.begin(), rules.end());
    while (mt_bits.size() % 32u) mt_bits.push_back(0xFFFFFFFFu);
    const uint32_t nr = (uint32_t)rules.size();
    // a wave's lane l zeroes / writes the site-record counters of the kernel's group l (groups have
    // 2+ members and a kernel at most KV_KROWS rules: at most 64 groups)
    if (kern.gsn > 64u) throw std::runtime_error("kvjit: more than 64 site-record groups in one kernel");
    std::ostringstream o;
    o << kern.decls;
    if (opt.stamps) o << "__device__ unsigned long long* kvj_stamps;\n";
    o << "__device__ const uint32_t " << name << "_rules[" << nr << "] = {";
    for (uint32_t q = 0; q < nr; q++) o << (q ? ", " : "") << u32(rules[q]);
    o << "};\n";
    // Occupancy over registers: the rule kernels are latency-bound on dependent
    // tree loads, so they ask for 8 waves per SIMD (<= 64 VGPRs) unless the plan
    // relaxes it for a kernel that would spill (jit_plan_spills).
    const std::string lb = waves > 0 ? "KV_RWG, " + std::to_string(waves) : "KV_RWG";
    o << "extern \"C\" __global__ __launch_bounds__(" << lb << ") void " << name
      << "(const DevPS* __restrict__ Pp, const DevBatch* __restrict__ Bp, const Node* __restrict__ N, "
         "const Val* __restrict__ V, const uint8_t* __restrict__ S, DevOut O, uint32_t r0) {\n"
      << "  constexpr uint32_t FIN_ = " << u32(FIN) << ", ACT_ = " << u32(ACT) << ", ST_STORED_ = 0x7Eu;\n"
      << "  __shared__ unsigned long long s_stq[" << kernel_lds(nr) / 8 + (KV_RWAVES * kern.gsn + 1u) / 2u
      << "];\n  uint32_t* s_stw = (uint32_t*)s_stq;\n"
      << "  const DevPS& P = *Pp;\n  const DevBatch& B = *Bp;\n  const uint8_t* __restrict__ pstr = P.pstr;\n";
    // Workgroup b runs tile (b % 8) * n/8 + b / 8, so each XCD (blocks b, b+8, ... share one)
    // walks a contiguous resource range and its L2 sees the values those resources share
    // (the value table and ptab lines are numbered by first occurrence): C2 -0.6 %, C3 -1 %
    // per pass, traffic -1 %
    o << "  const uint32_t nb_ = gridDim.x, x_ = blockIdx.x & 7u, per_ = nb_ >> 3, rem_ = nb_ & 7u;\n"
      << "  const uint32_t bx_ = x_ * per_ + (x_ < rem_ ? x_ : rem_) + (blockIdx.x >> 3);\n";
    o << "  const uint32_t r = r0 + bx_ * KV_RWG + threadIdx.x;\n"
      << "  const uint32_t n_res = B.n_res;\n"
      << "  const bool valid = r < n_res;\n"
      << "  const Res* __restrict__ R = B.res + (valid ? r : 0u);\n"
      << "  uint32_t root = ABSENT, rkind = KEY_NONE, rflags = 0u, rtup = 0u;\n"
      << "  if (valid) { root = ni(kv_gld(&R->root, 0)); rkind = kv_gld(&R->kind, 0); rflags = kv_gld(&R->flags, 0); rtup = kv_gld(&R->tup, 0); }\n"
      << "  Node rootn{0u, 0u, 0u, 0u};\n";
    // path columns (kvdevtypes.h): cell offset of this lane's family-0 columns; column 0 = the root
    o << "  const uint32_t* __restrict__ PC = B.pcol;\n"
        << "  const uint32_t ln_ = threadIdx.x & " << u32(KV_LANES - 1) << ", gw_ = (r >> 6) * KVC_W0;\n"
        << "  if (valid) rootn = " << col_macro("LD", 0, 0) << "(gw_);\n";
    o
      << "  const uint32_t* __restrict__ mtr_ = P.mtup + rtup;\n  const uint32_t ntup_ = B.n_tup;\n"
      << "  uint8_t* s_w = (uint8_t*)s_stw;\n"
      // every status row starts as NOMATCH (0xFF past the batch): only matched lanes store
      // site-record counters of the kernel's groups, [group][wave] after the rows (zeroed before
      // the prefill's barrier)
      << "  uint32_t* const s_gc_ = s_stw + " << u32(kernel_lds(nr) / 4u) << ";\n"
      << (kern.gsn ? "  for (uint32_t t_ = threadIdx.x; t_ < " + u32(KV_RWAVES * kern.gsn) + "; t_ += KV_RWG) s_gc_[t_] = 0u;\n"
                : std::string())
      << "  kv_prefill_rows(s_stw, " << nr << "u, r - threadIdx.x, n_res);\n";
    // diagnostics (KVGPU_JIT_STAMPS): a wave's shader clock at the start, after each block and
    // after the flush, into the program's global kvj_stamps ([workgroup][wave][kJitStamps], set by
    // kvapi.cpp)
    auto stamp = [&](size_t k) {
      if (opt.stamps && k < kJitStamps)
        o << "  if (kvj_stamps && (threadIdx.x & 63u) == 0u) kvj_stamps[((size_t)blockIdx.x * KV_RWAVES + (threadIdx.x >> 6)) * "
          << kJitStamps << "u + " << k << "u] = __builtin_amdgcn_s_memtime();\n";
    };
    stamp(0);
    for (size_t bi = 0; bi < blocks.size(); bi++) {
      // the block's match words (bits of its rules, kv_mtup_kernel); a wave none of whose resources
      // matches any rule of the block skips it whole (every rule NOMATCH on every lane)
      const uint32_t r0 = rows[bi].first, rn = rows[bi].second;
      const uint32_t p0 = kern.mt_kbase * 32u + r0, p1 = p0 + rn;  // bit positions [p0, p1)
      o << "  {\n";
      std::string any = "0u";
      for (uint32_t w = p0 / 32u; w * 32u < p1; w++) {
        const uint32_t lo = std::max(p0, w * 32u) - w * 32u, hi = std::min(p1, w * 32u + 32u) - w * 32u;
        const uint32_t m = hi - lo == 32u ? 0xFFFFFFFFu : ((1u << (hi - lo)) - 1u) << lo;
        o << "  const uint32_t mw" << w << " = valid ? kv_gld(mtr_, (size_t)" << w << "u * ntup_) : 0u;\n";
        any += " | (mw" + std::to_string(w) + " & " + u32(m) + ")";
      }
      // (the rows of a skipped block keep their NOMATCH prefill)
      o << "  if (__ballot((" << any << ") != 0u) != 0ull) {\n" << blocks[bi] << "  }\n";
      o << "  }\n";
      stamp(bi + 1);
    }
    // statuses to the status matrix, per-rule (and per-scope) histograms
    o << "  const uint32_t wg0_ = r - threadIdx.x;\n";
    // each wave's site-record counts (lane l: the kernel's group l)
    if (kern.gsn)
      o << "#ifndef KVEMU\n  if ((KV_OFULL(O) & 2u) && !(KV_OFULL(O) & 4u) && (threadIdx.x & 63u) < " << u32(kern.gsn)
        << " && r - (threadIdx.x & 63u) < n_res)\n    O.gcnt[(size_t)(" << u32(kern.gs0)
        << " + (threadIdx.x & 63u)) * ((n_res + 63u) >> 6) + (r >> 6)] = s_gc_[(threadIdx.x & 63u) * KV_RWAVES + (threadIdx.x >> 6)];\n#endif\n";
    o << "  kv_end_flush<" << nr << "u>(O, s_stw, " << name << "_rules, n_res, r, valid, "
         "(KV_OFULL(O) & 8u) && valid ? O.scope[r] : 0xFFFFFFFFu, (KV_OFULL(O) & 8u) && wg0_ < n_res ? O.scope[wg0_] : 0xFFFFFFFFu, "
         "P.n_rules);\n";
    stamp(std::min<size_t>(blocks.size() + 1, kJitStamps - 1));
    o << "}\n\n";
    kernels.push_back({name, o.str()});
    return rules;
  }

  // Factored match descriptors (DevPS::fac_*, kv_mfac / kv_mtup in kvkernel.hip) for the
  // match bits of every rule in kernel order. A rule's match is an OR of planes minus an OR
  // of exclude planes (rule_matches, kvdevfn.h): `any` blocks give one plane per filter,
  // `all` blocks one plane of all their filters, a legacy block one plane of its filter. A
  // word takes as many match / exclude planes as its widest rule; rules with name filters
  // keep their per-resource bit, rules with more than KV_FAC_MAXP planes run rule_matches per
  // tuple.
  void build_fac(JitImage* out) const {
    const uint32_t W = (uint32_t)(mt_bits.size() / 32u);
    out->fac_word.assign(4u * W, 0u);
    out->fac_bit.clear();
    out->fac_flist.clear();
    out->fac_rule = mt_bits;
    auto planes = [&](uint32_t mode, uint32_t first, uint32_t count) {
      std::vector<std::vector<uint32_t>> p;
      if (mode == 1) {
        for (uint32_t f = first; f < first + count; f++) p.push_back({f});
      } else if (mode == 2) {
        std::vector<uint32_t> all;
        for (uint32_t f = first; f < first + count; f++) all.push_back(f);
        p.push_back(all);
      } else {
        p.push_back({first});
      }
      return p;
    };
    uint32_t slot = 0;
    for (uint32_t w = 0; w < W; w++) {
      std::vector<std::vector<std::vector<uint32_t>>> mp(32), xp(32);
      uint32_t nm = 0, nx = 0, named = 0, cx = 0;
      for (uint32_t b = 0; b < 32u; b++) {
        const uint32_t ri = mt_bits[w * 32u + b];
        if (ri == 0xFFFFFFFFu) continue;
        if (name_dependent(ri)) {
          named |= 1u << b;
          continue;
        }
        const RuleRec& rr = ps.rules[ri];
        auto m = planes(rr.m_mode, rr.m_first, rr.m_count), x = planes(rr.x_mode, rr.x_first, rr.x_count);
        if (m.size() > KV_FAC_MAXP || x.size() > KV_FAC_MAXP) {
          cx |= 1u << b;
          continue;
        }
        nm = std::max<uint32_t>(nm, (uint32_t)m.size());
        nx = std::max<uint32_t>(nx, (uint32_t)x.size());
        mp[b] = std::move(m);
        xp[b] = std::move(x);
      }
      out->fac_word[4u * w] = slot;
      out->fac_word[4u * w + 1] = nm | nx << 8;
      out->fac_word[4u * w + 2] = named;
      out->fac_word[4u * w + 3] = cx;
      for (uint32_t p = 0; p < nm + nx; p++, slot++)
        for (uint32_t b = 0; b < 32u; b++) {
          const auto& pl = p < nm ? mp[b] : xp[b];
          const uint32_t k = p < nm ? p : p - nm;
          if (k < pl.size()) {
            out->fac_bit.push_back((uint32_t)out->fac_flist.size());
            out->fac_bit.push_back((uint32_t)pl[k].size() | KV_FAC_PRESENT);
            out->fac_flist.insert(out->fac_flist.end(), pl[k].begin(), pl[k].end());
          } else {
            out->fac_bit.push_back(0u);
            out->fac_bit.push_back(0u);
          }
        }
    }
    out->fac_slots = slot;
    if (out->fac_flist.empty()) out->fac_flist.push_back(0u);
    if (out->fac_bit.empty()) out->fac_bit.assign(2, 0u);
  }

  // Register weight of rule ri in a fused block: the state it keeps across the block (status
  // / resume pc, error kind, cursors per depth, loop counters and error indices per loop
  // level, anchor bitsets, wildcard-key node); 0 for rules of other routes.
  uint32_t rule_weight(uint32_t ri) {
    if (no_program(ps.rules[ri])) return 0;
    const RGen g = analyze(ri);
    uint32_t w = 2 + g.maxd;
    if (!g.loops.empty()) w += 4 * (g.max_level + 1);
    if (g.uses_anchor) w += 4;
    if (g.uses_keyglob) w += 3;
    return w;
  }

  // First block sizes of the kernel of sorted rules [a, e): greedy runs whose weight stays
  // within a budget (KVGPU_JIT_BLOCK_W, default 160, see below); a rule of the same structural
  // form as an earlier rule of the run joins it for free (rule groups run its program once).
  // A kernel the default budget cuts into many blocks is cut again with 1.5x the budget: it
  // re-walks its resources once per block, and the block probes still split whatever does not
  // fit its registers (round 4, gpurun_out/ab9 / ab8, ms per pass: C5 3.45 -> 3.25, C4 1.00 ->
  // 0.99; C2, three blocks, keeps the default: with 1.5x 0.694 -> 0.712).
  std::vector<uint32_t> initial_blocks(const std::vector<uint32_t>& sorted, uint32_t a, uint32_t e) {
    if (opt.block_w) return initial_blocks_w(sorted, a, e, opt.block_w);
    std::vector<uint32_t> out = initial_blocks_w(sorted, a, e, 160u);
    if (out.size() >= 6) out = initial_blocks_w(sorted, a, e, 240u);
    return out;
  }
  std::vector<uint32_t> initial_blocks_w(const std::vector<uint32_t>& sorted, uint32_t a, uint32_t e, uint32_t budget) {
    std::vector<uint32_t> out;
    std::set<std::string> seen;  // forms of the run
    uint32_t cur = 0, w = 0;
    for (uint32_t q = a; q < e; q++) {
      const uint32_t ri = sorted[q];
      const std::string& f = form_of(ri).text;
      const uint32_t rw = rule_weight(ri);
      if (cur > 0 && w + (seen.count(f) ? 0u : rw) > budget) {  // the run is full: a new one
        out.push_back(cur);
        cur = 0;
        w = 0;
        seen.clear();
      }
      cur++;
      if (!seen.count(f)) w += rw;
      if (!f.empty()) seen.insert(f);
    }
    if (cur) out.push_back(cur);
    return out;
  }
};

// Sort key grouping rules with the same walk: the symbolic path of the first
// top-level array loop, then the sorted paths of the leaves it tests.
std::string rule_signature(const PolicySet& ps, uint32_t ri) {
  std::vector<std::string> expr(64);
  expr[0] = "R";
  std::string arr;
  std::vector<std::string> leaves;
  int nest = 0;
  for (uint32_t pc = ps.rules[ri].prog;; pc++) {
    const Inst& in = ps.prog[pc];
    const uint32_t op = in.op & 0xFF, d = (in.op >> 8) & 0xFF, aux = (in.op >> 16) & 0xFF;
    if (op == OP_DONE || d + 1 >= expr.size()) break;
    switch (op) {
      case OP_KEY:
      case OP_KEYV:
        expr[d + 1] = expr[d].empty() ? "" : expr[d] + ((aux & AUX_SCAN) ? "/k" : "/s") + std::to_string(in.a);
        break;
      case OP_LEAF:
        leaves.push_back(expr[d]);
        break;
      case OP_LOOP_BEGIN:
      case OP_EXIST_BEGIN:
        if (op == OP_LOOP_BEGIN && nest == 0 && arr.empty()) {
          arr = expr[d].empty() ? "?" : expr[d];
          expr[d + 1] = "E";
        } else {
          expr[d + 1].clear();
        }
        nest++;
        break;
      case OP_LOOP_END:
      case OP_EXIST_END:
        nest--;
        break;
      case OP_KEYGLOB:
      case OP_INDEX:
        expr[d + 1].clear();
        break;
      default:
        break;
    }
  }
  std::sort(leaves.begin(), leaves.end());
  std::string sig = (arr.empty() ? "~" : arr) + "|";
  for (auto& l : leaves) sig += l + ",";
  return sig;
}

// The kinds rule ri's match blocks admit ("*" when any block admits every kind): rules of
// one kind set then share blocks, which the kind-grouped store order lets whole waves skip
std::string rule_kind_key(const PolicySet& ps, uint32_t ri) {
  const RuleRec& rr = ps.rules[ri];
  std::vector<std::string> ks;
  for (uint32_t f = rr.m_first; f < rr.m_first + rr.m_count; f++) {
    const MFilter& F = ps.filters[f];
    if (!(F.flags & MF_KINDS)) return "*";
    for (uint32_t i = F.kinds_first; i < F.kinds_first + F.kinds_count; i++) {
      const KindSpec& k = ps.kinds[i];
      if (k.form == 3) return "*";
      ks.push_back(std::to_string(k.kind));
    }
  }
  std::sort(ks.begin(), ks.end());
  ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
  std::string key;
  for (auto& k : ks) key += k + ",";
  return key;
}

// The rules in kernel order: rules that walk the same arrays and leaves share a kernel (and its
// hoisted lookups). Grouped by the kinds they match first, walk signature second (round 3: C5
// 4.07 -> 3.72 ms against signature only, C3 10.19 -> 10.32); rules without a program last.
std::vector<uint32_t> rule_order(const PolicySet& ps) {
  std::vector<std::pair<std::string, uint32_t>> order;
  for (uint32_t ri = 0; ri < ps.rules.size(); ri++)
    order.push_back({!no_program(ps.rules[ri]) ? "0" + rule_kind_key(ps, ri) + "#" + rule_signature(ps, ri) : "1", ri});
  std::stable_sort(order.begin(), order.end());
  std::vector<uint32_t> sorted;
  for (auto& o : order) sorted.push_back(o.second);
  return sorted;
}

// The first plan: one kernel per range of the rule order, ceil(n / chunk_rules) ranges of
// near-equal size, each cut into its first blocks (Gen::initial_blocks).
// KVGPU_JIT_WAVES: launch bound in waves per SIMD (default 8, 0: none)
std::vector<JitKernelPlan> first_plan(Gen& g, const std::vector<uint32_t>& sorted, uint32_t chunk_rules) {
  // first bound: about 160 KB / (256 B x rules) waves, at most 8 and at most what the
  // kernel's LDS (kernel_lds) leaves of a CU's 160 KB (one workgroup = one wave per SIMD);
  // the spill plan splits blocks (or lowers the bound) until the compiler meets it. A kernel
  // of many rules keeps more state live across its fused blocks, and trading occupancy for
  // fewer, larger blocks (fewer walks of the resource tree) wins there: C2 (100 rules, one
  // kernel) 6 waves 4 blocks 0.697 ms, 7 waves 16 blocks 0.902 ms, 8 waves 35 blocks
  // 1.224 ms per pass (round 4, gpurun_out/r4b/ab); C4's ~70-rule kernels run at 8.
  const uint32_t n = (uint32_t)sorted.size();
  if (chunk_rules == 0 || chunk_rules > KV_KROWS) chunk_rules = KV_KROWS;
  uint32_t parts = (n + chunk_rules - 1) / chunk_rules;
  // one more range while the longest ranges would get fewer workgroups per CU than the
  // shortest (C3: 1 973 rules in 16 ranges of 123/124 -> 17 of 116/117)
  while (parts < n && Gen::lds_waves((n + parts - 1) / parts) < Gen::lds_waves(n / parts)) parts++;
  std::vector<JitKernelPlan> plan;
  for (uint32_t k = 0; k < parts; k++) {
    const uint32_t a = (uint32_t)((uint64_t)n * k / parts), e = (uint32_t)((uint64_t)n * (k + 1) / parts);
    std::vector<uint32_t> bl = g.initial_blocks(sorted, a, e);
    // workgroups of 4 waves: waves per SIMD = workgroups per CU the LDS admits
    const int lds_waves = Gen::lds_waves(e - a);
    const int rule_waves = (int)std::max<uint32_t>(1u, (160u * 1024u) / std::max<uint32_t>(1u, (e - a) * 256u));
    plan.push_back({a, e - a, g.opt.has_waves ? g.opt.waves : std::min({8, lds_waves, rule_waves}), bl, true, true});
  }
  return plan;
}

// Each kernel program = the column macros + the helper functions it reaches + the kernel: the
// helpers (Gen::helpers, one record per function) are selected by a transitive scan of the names
// they use and kept in generation order (which is dependency order). out->source: all of it.
void assemble_programs(const Gen& g, const std::string& prelude, const std::string& cdefs, JitImage* out) {
  const std::vector<std::pair<std::string, std::string>>& defs = g.helpers;  // (name, text)
  std::unordered_map<std::string, size_t> def_index;
  for (size_t i = 0; i < defs.size(); i++) def_index[defs[i].first] = i;
  auto refs = [&](const std::string& text, std::vector<size_t>* out_ids) {
    static const char* prefixes[] = {"g_glob_", "g_atom_", "g_pred_", "g_blk_", "g_match_",
                                     "g_dleaf_", "q_glob_", "q_atom_", "q_pred_", "r_glob_", "r_atom_", "r_pred_"};
    for (const char* pf : prefixes) {
      const size_t pl = strlen(pf);
      for (size_t q = text.find(pf); q != std::string::npos; q = text.find(pf, q + pl)) {
        size_t e = q + pl;
        while (e < text.size() && isdigit((unsigned char)text[e])) e++;
        auto it = def_index.find(text.substr(q, e - q));
        if (it != def_index.end()) out_ids->push_back(it->second);
      }
    }
  };
  out->common = prelude;
  out->kernel_name.clear();
  out->kernel_src.clear();
  out->source = prelude + cdefs;
  for (const auto& d : defs) out->source += d.second;
  for (auto& k : g.kernels) {
    std::vector<char> used(defs.size(), 0);
    std::vector<size_t> stack;
    refs(k.second, &stack);
    while (!stack.empty()) {
      const size_t d = stack.back();
      stack.pop_back();
      if (used[d]) continue;
      used[d] = 1;
      refs(defs[d].second, &stack);
    }
    std::string prog;
    for (size_t d = 0; d < defs.size(); d++)
      if (used[d]) prog += defs[d].second;
    out->kernel_name.push_back(k.first);
    out->kernel_src.push_back(cdefs + prog + k.second);
    out->source += k.second;
  }
}

}  // namespace

uint32_t jit_chunk_rules() {
  const char* ch = getenv("KVGPU_JIT_CHUNK");
  // (at most KV_KROWS: the kernels' record counters have a byte per (wave, rule))
  return ch && atoi(ch) > 0 ? std::min<uint32_t>((uint32_t)atoi(ch), KV_KROWS) : KV_KROWS;
}

void jit_generate(const PolicySet& ps, uint32_t chunk_rules, JitImage* out) {
  auto t0 = std::chrono::steady_clock::now();
  Gen g(ps);
  g.use_seed = out->col_use;
  const std::string prelude =
      g.opt.diag + kPrelude + std::string("\nusing namespace kv;\n\n") +
      "__device__ __noinline__ bool kv_dleaf_impl(const DevBatch& B, const Node* __restrict__ N, uint32_t dp, Node vn);\n\n";
  for (uint32_t ri = 0; ri < ps.rules.size(); ri++)
    if (!no_program(ps.rules[ri])) g.leaf_classes(ri);
  for (uint32_t ri = 0; ri < ps.rules.size(); ri++) g.match_fn(ri);
  out->chunks.clear();
  const uint32_t n = (uint32_t)ps.rules.size();
  const std::vector<uint32_t> sorted = rule_order(ps);
  if (out->plan.empty() && n) out->plan = first_plan(g, sorted, chunk_rules);
  for (const JitKernelPlan& kp : out->plan) {
    JitChunk kc;
    // named by its rule range and block count: stable when other ranges are re-planned
    kc.name = "kvj_r" + std::to_string(kp.first) + "_" + std::to_string(kp.count) +
              (kp.blocks.size() > 1 ? "_b" + std::to_string(kp.blocks.size()) : "") + (kp.waves ? "" : "u");
    for (uint32_t q = kp.first; q < kp.first + kp.count; q++) kc.rules.push_back(sorted.at(q));
    std::vector<std::vector<uint32_t>> bl;
    uint32_t at = 0;
    for (uint32_t c : kp.blocks) {
      if (at + c > kp.count) break;
      bl.emplace_back(kc.rules.begin() + at, kc.rules.begin() + at + c);
      at += c;
    }
    if (at != kp.count) throw std::runtime_error("kvjit: kernel plan blocks do not cover its rules");
    // the kernel's rules in LDS-row order (blocks reorder rule-group members)
    kc.rules = g.group_kernel(kc.name, bl, kp.waves, kp.grouped, kp.colloops);
    out->chunks.push_back(kc);
  }
  out->mtup_words = (uint32_t)(g.mt_bits.size() / 32u);
  if (out->mtup_words && !out->probe) g.build_fac(out);
  out->rec_compact.assign(n, 1);
  for (uint32_t ri = 0; ri < n; ri++) out->rec_compact[ri] = g.rec_slot[ri] ? 0 : 1;
  out->gs_desc = g.gs_desc;
  out->gs_mem = g.gs_mem;
  out->gs_members = g.gs_members;
  std::string cdefs;  // the row words of every path-column family and the macros of every column
  g.col_plan(out, &cdefs);

  out->memo_preds.clear();
  out->memo_words = 0;
  if (!g.mpreds.empty() && !out->probe) {
    g.ptab_kernel();
    out->memo_preds = g.mpreds;
    out->memo_words = (uint32_t)((g.mpreds.size() + 31) / 32);
    out->ptab_row = g.ptab_row_out();
  }
  assemble_programs(g, prelude, cdefs, out);
  out->gen_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace kvh
