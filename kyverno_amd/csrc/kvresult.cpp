// Host-side reading of a fetched result (kv_result, ResultPart): the status matrix from the
// transfer form, records, failing paths and messages, the bulk failure export, and the entry
// points that only read host tables. Includes no HIP header and calls no HIP function: the host
// harness (tools/kvemu) builds this file under ASan/UBSan.
#include <emmintrin.h>

#include <algorithm>
#include <cassert>
#include <cstring>
#include <unordered_map>

#include "kvrt.hpp"

void ResultPart::unpack_row(uint32_t rule, uint8_t* dst) const {
  if (!n || sbase.empty()) return;  // (a part without resources packs nothing)
  const uint8_t* f = sflag.data() + (size_t)rule * nwg;
  const uint8_t* src = spack.data() + sbase[rule] * (KV_RWG / 2);
  const __m128i lo4 = _mm_set1_epi8(0x0F);
  for (uint64_t g = 0; g < nwg; g++) {
    const uint64_t q0 = g * KV_RWG, m = std::min<uint64_t>(KV_RWG, n - q0);
    uint8_t* d = dst + q0;
    if (!f[g]) {
      memset(d, ST_NOMATCH, m);
      continue;
    }
    uint64_t i = 0;
    for (; i + 32 <= m; i += 32) {
      const __m128i b = _mm_loadu_si128((const __m128i*)(src + i / 2));
      const __m128i l = _mm_and_si128(b, lo4), h = _mm_and_si128(_mm_srli_epi16(b, 4), lo4);
      _mm_storeu_si128((__m128i*)(d + i), _mm_unpacklo_epi8(l, h));
      _mm_storeu_si128((__m128i*)(d + i + 16), _mm_unpackhi_epi8(l, h));
    }
    for (; i < m; i++) d[i] = (src[i / 2] >> (4 * (i & 1))) & 15u;
    src += KV_RWG / 2;
  }
}

void kv_result::gather_row(const uint8_t* row, const uint32_t* inv, uint64_t n, uint8_t* out) {
  uint64_t c = 0;
  for (; c + 8 <= n; c += 8) {
    uint64_t v = 0;
    for (int k = 0; k < 8; k++) v |= (uint64_t)row[inv[c + k]] << (8 * k);
    memcpy(out + c, &v, 8);
  }
  for (; c < n; c++) out[c] = row[inv[c]];
}

void kv_result::unpack_rows(uint8_t* dst, const uint32_t* inv) const {
  const unsigned T = host_threads();
  std::vector<std::thread> th;
  for (unsigned t = 0; t < T; t++)
    th.emplace_back([&, t]() {
      std::vector<uint8_t> tmp(inv ? n_res : 0);
      for (uint64_t rl = t; rl < n_rules; rl += T) {
        uint8_t* row = inv ? tmp.data() : dst + rl * n_res;
        for (const ResultPart& p : parts) p.unpack_row((uint32_t)rl, row + p.lo);
        if (inv) gather_row(row, inv, n_res, dst + rl * n_res);
      }
    });
  for (auto& x : th) x.join();
}

const uint8_t* kv_result::st_store() {
  if (sparse)
    std::call_once(st_once, [this]() {
      status.alloc(n_rules * n_res);
      unpack_rows(status.data(), nullptr);
    });
  return status.empty() ? nullptr : status.data();
}

const uint8_t* kv_result::status_caller() {
  if (b->b.order.empty() || !has_status() || caller_order) return st_store();
  std::call_once(sc_once, [this]() {
    status_c.alloc(n_rules * n_res);
    const uint32_t* inv = const_cast<kv_batch*>(b)->inverse();
    if (status.empty()) {
      unpack_rows(status_c.data(), inv);
      return;
    }
    const unsigned T = host_threads();
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; t++)
      th.emplace_back([&, t]() {
        for (uint64_t rl = t; rl < n_rules; rl += T)
          gather_row(status.data() + rl * n_res, inv, n_res, status_c.data() + rl * n_res);
      });
    for (auto& x : th) x.join();
  });
  return status_c.data();
}

ErrRec kv_result::decode(const ErrRec8& c) {
  ErrRec e{};
  e.kind_flags = (c.w0 & 15u) | (((c.w0 >> 4) & 3u) << 16);
  e.pnode = c.w0 >> 7;
  e.keynode = ABSENT;
  e.resnode = ABSENT;
  e.idx[0] = c.w1 & 1023u;
  e.idx[1] = (c.w1 >> 10) & 255u;
  e.idx[2] = (c.w1 >> 18) & 255u;
  e.idx[3] = 0;
  return e;
}

uint64_t kv_result::rec_index(const ResultPart& p, uint32_t rule, uint64_t res) const {
  const uint64_t local = res - p.lo;
  const uint64_t tile = local / KV_WG;
  uint64_t idx = p.base[rule] + p.offs[(size_t)rule * p.tiles + tile];
  const uint8_t* row = const_cast<kv_result*>(this)->st_store() + (size_t)rule * n_res;
  for (uint64_t q = p.lo + tile * KV_WG; q < res; q++) {
    const uint8_t s = row[q];
    idx += s == ST_FAIL || s == ST_ERROR || s == ST_SKIP;
  }
  return idx;
}

bool kv_result::err(uint32_t rule, uint64_t res, ErrRec* e, const Batch** bt) const {
  const ResultPart* p = part_of(res);
  if (!p || !errors) return false;
  const uint64_t i = rec_index(*p, rule, res);
  if (i >= p->n_rec() || i < p->base[rule] || i >= p->base[rule + 1]) return false;
  const ErrRec8 c = p->r8(rule, i);
  *e = (c.w0 & ERR8_WIDE) && !p->recw.empty() ? p->recw[i] : decode(c);
  *bt = &batch_of(*p);
  return true;
}

int kvh::fail(kv_error** err, int code, const std::string& msg) {
  if (err) {
    *err = (kv_error*)malloc(sizeof(kv_error));
    (*err)->code = code;
    (*err)->message = strdup(msg.c_str());
  }
  return code;
}

namespace {

// Path segments from the pattern root to pnode p: keys (resolved wildcard keys
// from the record's key node) and array indices (loop counters of the record).
struct PathSeg {
  bool index;
  std::string key;
};
std::vector<PathSeg> path_segs(const PolicySet& ps, const Batch& b, const ErrRec& e, uint32_t p) {
  std::vector<PathSeg> segs;
  while (p != 0xFFFFFFFFu && p < ps.pnodes.size()) {
    const PNodeInfo& n = ps.pnodes[p];
    switch (n.seg) {
      case SEG_ROOT: break;
      case SEG_KEY: segs.push_back({false, n.key}); break;
      case SEG_LOOP: segs.push_back({true, std::to_string(e.idx[n.level & 3])}); break;
      case SEG_CONST_INDEX: segs.push_back({true, std::to_string(n.level)}); break;
      case SEG_RESOLVED: {
        if (e.keynode != ABSENT && e.keynode < b.n_cells()) {
          uint32_t k = node_key(b.cell(e.keynode).kt);
          segs.push_back({false, k < ps.keys.size() ? ps.keys[k] : b.dyn_keys[k - ps.keys.size()]});
        } else {
          segs.push_back({false, n.key});
        }
        break;
      }
    }
    p = n.parent;
  }
  std::reverse(segs.begin(), segs.end());
  return segs;
}

std::string join_path(const std::vector<PathSeg>& segs) {
  std::string out = "/";
  for (const PathSeg& s : segs) out += s.key + "/";
  return out;
}

uint32_t err_kind(const ErrRec& e) { return e.kind_flags & 0xFFFF; }

// pnode whose path is the PatternError path: the "*" shortcut reports its parent
// map (anchor.go:139), every other form the node it was raised at
uint32_t path_pnode(const PolicySet& ps, const ErrRec& e) {
  if (err_kind(e) == E_STAR && e.pnode < ps.pnodes.size()) return ps.pnodes[e.pnode].parent;
  return e.pnode;
}

std::string render_path(const PolicySet& ps, const Batch& b, const ErrRec& e) {
  return join_path(path_segs(ps, b, e, path_pnode(ps, e)));
}

// ---- Go fmt of resource values (unstructured typing: int64 / float64 / string /
// bool / nil / map[string]interface{} / []interface{}), for '%v' and %T operands
std::string res_T(const JDoc& d, int64_t n) {
  if (n < 0) return "<nil>";
  switch (d.at((uint32_t)n).t) {
    case J_MAP: return "map[string]interface {}";
    case J_ARR: return "[]interface {}";
    case J_STR: return "string";
    case J_BOOL: return "bool";
    case J_INT: return "int64";
    case J_FLOAT: return "float64";
    default: return "<nil>";
  }
}

std::string res_v(const JDoc& d, int64_t n) {
  if (n < 0) return "<nil>";
  const JNode& x = d.at((uint32_t)n);
  switch (x.t) {
    case J_MAP: {  // fmt prints maps with sorted keys
      std::vector<uint32_t> ix;
      for (uint32_t c = x.first; c < x.first + x.count; c++) ix.push_back(c);
      std::sort(ix.begin(), ix.end(), [&](uint32_t a, uint32_t b) { return d.key(d.at(a)) < d.key(d.at(b)); });
      std::string o = "map[";
      for (size_t k = 0; k < ix.size(); k++) {
        if (k) o += ' ';
        o += d.key(d.at(ix[k]));
        o += ':';
        o += res_v(d, ix[k]);
      }
      return o + "]";
    }
    case J_ARR: {
      std::string o = "[";
      for (uint32_t c = x.first; c < x.first + x.count; c++) {
        if (c > x.first) o += ' ';
        o += res_v(d, c);
      }
      return o + "]";
    }
    case J_STR: return std::string(d.sval(x));
    case J_BOOL: return x.b ? "true" : "false";
    case J_INT: return std::to_string(x.i);
    case J_FLOAT: return go_format_g(x.f);
    default: return "<nil>";
  }
}

// resource element at a pattern path (-1 when absent)
int64_t res_at(const JDoc& d, const std::vector<PathSeg>& segs) {
  int64_t n = d.root;
  for (const PathSeg& s : segs) {
    if (n < 0) return -1;
    const JNode& x = d.at((uint32_t)n);
    if (x.t == J_MAP) {
      n = d.get((uint32_t)n, s.key);
    } else if (x.t == J_ARR && s.index) {
      uint64_t i = std::stoull(s.key);
      n = i < x.count ? (int64_t)(x.first + i) : -1;
    } else {
      return -1;
    }
  }
  return n;
}

// err.Error() of the PatternError behind a FAIL / ERROR / SKIP record
// (pkg/engine/validate/validate.go:62-172, pkg/engine/anchor/anchor.go:61-261;
// condition / global anchor handlers wrap what propagates through them,
// anchor.go:72-95 with common/anchorKey.go:21-40)
std::string error_message(const PolicySet& ps, const Batch& b, const ErrRec& e, const JDoc& doc,
                          const std::string* dyn_pat_v = nullptr) {
  const uint32_t kind = err_kind(e);
  if (e.pnode >= ps.pnodes.size()) return "";
  PNodeInfo P = ps.pnodes[e.pnode];
  // the resource's (a foreach entry's pattern: the element's) substituted pattern value
  if ((P.dleaf >= 0 || P.fe_key >= 0) && dyn_pat_v) P.pat_v = *dyn_pat_v;
  const std::vector<PathSeg> segs = path_segs(ps, b, e, e.pnode);
  const std::string path = join_path(segs);
  std::string m;
  switch (kind) {
    case E_TYPE_MAP:
      m = "pattern and resource have different structures. Path: " + path + ". Expected " + P.pat_t + ", found " +
          res_T(doc, res_at(doc, segs));
      break;
    case E_TYPE_ARR:
      m = "validation rule Failed at path " + path + ", resource does not satisfy the expected overlay pattern";
      break;
    case E_VALUE:
      m = "resource value '" + res_v(doc, res_at(doc, segs)) + "' does not match '" + P.pat_v + "' at path " + path;
      break;
    case E_EMPTY_PATARR: m = "pattern Array empty"; break;
    case E_LEN: {
      int64_t n = res_at(doc, segs);
      uint32_t rl = n >= 0 && doc.at((uint32_t)n).t == J_ARR ? doc.at((uint32_t)n).count : 0;
      m = "validate Array failed, array length mismatch, resource Array len is " + std::to_string(rl) +
          " and pattern Array len is " + std::to_string(P.pat_len);
      break;
    }
    case E_NEG: m = path + "/" + (segs.empty() ? std::string() : segs.back().key) + " is not allowed"; break;
    case E_STAR: {
      std::vector<PathSeg> ps_ = segs;
      std::string key = ps_.empty() ? std::string() : ps_.back().key;
      if (!ps_.empty()) ps_.pop_back();
      m = join_path(ps_) + "/" + key + " not found";
      break;
    }
    case E_EXIST_PATLIST:
      m = "invalid pattern type " + P.pat_t + ": Pattern has to be of list to compare against resource";
      break;
    case E_EXIST_PATMAP:
      m = "invalid pattern type " + P.pat_t + ": Pattern has to be of type map to compare against items in resource";
      break;
    case E_EXIST_RESTYPE:
      m = "invalid resource type " + res_T(doc, res_at(doc, segs)) +
          ": Existence ^ () anchor can be used only on list/array type resource";
      break;
    case E_EXIST_FAIL: m = "existence anchor validation failed at path " + path; break;
    default: return "";
  }
  for (uint32_t q = e.pnode; q != 0xFFFFFFFFu && q < ps.pnodes.size(); q = ps.pnodes[q].parent) {
    if (ps.pnodes[q].wrap == 1) m = "conditional anchor mismatch: " + m;
    else if (ps.pnodes[q].wrap == 2) m = "global anchor mismatch: " + m;
  }
  return m;
}

// a message into the caller's buffer (truncated to cap - 1 bytes); returns its full length
int put_message(const std::string& m, char* buf, size_t cap) {
  if (buf && cap) {
    size_t n = std::min(cap - 1, m.size());
    memcpy(buf, m.data(), n);
    buf[n] = 0;
  }
  return (int)m.size();
}

// One (rule, caller resource) pair of a result, resolved once for every per-pair accessor: the
// index of its status and record (`sx`, in the result's order), its store slot (`s`, the order of
// the batch-side tables), the part, the batch or shard that owns the slot and the slot's index
// there. Invariant: a caller_order result has exactly one part, starting at 0 (DevSession::fetch
// reorders only a permuted batch fetched whole), so part_of(sx) and part_of(s) are the same part.
struct Pair {
  int code = 0;  // KV_E_INVALID / KV_E_RANGE: no such pair, nothing else is set
  kv_result* r = nullptr;
  uint32_t rule = 0;
  uint64_t sx = 0, s = 0, local = 0;
  const ResultPart* part = nullptr;  // (null: no part holds the slot; kb is null too)
  kv_batch* kb = nullptr;
  const PolicySet& ps() const { return *r->ps; }
  uint64_t n_local() const { return kb->b.res.size(); }
  // the pair's status, on demand: it materialises the status matrix of a packed result, so an
  // accessor tests what it can tell from the rule alone first
  uint8_t status() const { return r->st_store()[(size_t)rule * r->n_res + sx]; }
  bool record(ErrRec* e, const Batch** bt) const { return r->err(rule, sx, e, bt); }
};

// `records`: the accessor reads error records (a result fetched with KV_MODE_ERRORS), else statuses
Pair pair_of(const kv_result* cr, uint32_t rule, uint64_t res, bool records) {
  Pair q;
  if (!cr || (records && !cr->has_err())) q.code = KV_E_INVALID;
  else if (rule >= cr->n_rules || res >= cr->n_res) q.code = KV_E_RANGE;
  else if (!records && !cr->has_status()) q.code = KV_E_INVALID;  // counts-only result: no statuses were fetched
  if (q.code) return q;
  assert(!cr->caller_order || (cr->parts.size() == 1 && cr->parts[0].lo == 0));
  q.r = const_cast<kv_result*>(cr);
  q.rule = rule;
  q.s = cr->store_of(res);
  q.sx = cr->caller_order ? res : q.s;
  if ((q.part = cr->part_of(q.s)) != nullptr) {
    q.kb = q.part->shard ? q.part->shard.get() : const_cast<kv_batch*>(cr->b);
    q.local = q.s - q.part->lo;
  }
  return q;
}

bool is_record(uint8_t st) { return st == ST_FAIL || st == ST_ERROR || st == ST_SKIP; }

// A pair of a device foreach rule with a pattern entry (KV_COMPILE_FOREACH_PATTERN) whose status
// its deciding element gave: the fetched reduction key and that element's record. False for every
// other pair (another rule, no fetched rows, a status the rule's own preconditions or match
// decided, PASS / SKIP).
// The fetched chain key of a pair of a rule of several entries (KV_COMPILE_FOREACH_ENTRIES;
// kvforeach.h kv_fe_chain). False for every other rule and without fetched rows.
bool chain_key(const Pair& q, uint32_t* key) {
  const uint32_t ch = q.ps().rhost[q.rule].foreach_chain;
  if (!ch || !q.part || q.part->fe_ckey.empty()) return false;
  *key = q.part->fe_ckey[(size_t)(ch - 1) * q.part->n + q.local];
  return true;
}

// The entry that decided a FAIL / ERROR pair of a device foreach rule: its foreach set, its
// position among the rule's entries (0 for a rule of one entry) and, for a rule of several
// entries, the deciding element (else 0xFFFFFFFF: the callers find it per set kind). False where
// the fold did not decide the pair.
bool deciding_entry(const Pair& q, uint8_t st, uint32_t* set, uint32_t* entry, uint32_t* elem) {
  const RuleHost& rh = q.ps().rhost[q.rule];
  *elem = 0xFFFFFFFFu;
  if (rh.foreach_set) {
    *set = rh.foreach_set - 1;
    *entry = 0;
    return q.part != nullptr;
  }
  uint32_t k;
  if (!chain_key(q, &k) || k >= FE_KEY_PASS || (k & 7u) != st) return false;
  const std::vector<uint32_t>& c = q.ps().fe_chains[rh.foreach_chain - 1];
  if ((k >> 19) >= c.size()) return false;
  *entry = k >> 19;
  *set = c[*entry];
  *elem = (k >> 3) & 0xFFFFu;
  return true;
}

bool pattern_pair(const Pair& q, uint32_t* key, ErrRec8* rec) {
  if (!q.part || q.part->fe_key.empty()) return false;
  const RuleHost& rh = q.ps().rhost[q.rule];
  if (!rh.foreach_set && !rh.foreach_chain) return false;
  const uint8_t st = q.status();
  if (st != ST_FAIL && st != ST_ERROR) return false;
  uint32_t set, entry, elem;
  if (!deciding_entry(q, st, &set, &entry, &elem) || !q.ps().fsets[set].pattern) return false;
  const size_t at = (size_t)q.ps().fsets[set].pat * q.part->n + q.local;
  const uint32_t k = q.part->fe_key[at];
  if (k >= FE_KEY_PASS || (k & 7u) != st) return false;
  if (rh.foreach_chain && (k >> 3) != elem) return false;
  *key = k;
  *rec = q.part->fe_rec[at];
  return true;
}

// A FAIL pair of a device foreach rule that an anyPattern entry decided
// (KV_COMPILE_FOREACH_ANYPATTERN): the fetched reduction key, the deciding element's code word, the
// deciding set and the row of its first alternative in fe_arec. False for every other pair.
bool any_pair(const Pair& q, uint32_t* key, uint32_t* cw, uint32_t* set_o, size_t* alt0) {
  if (!q.part || q.part->fe_akey.empty()) return false;
  const RuleHost& rh = q.ps().rhost[q.rule];
  if (!rh.foreach_set && !rh.foreach_chain) return false;
  const uint8_t st = q.status();
  if (st != ST_FAIL) return false;
  uint32_t set, entry, elem;
  if (!deciding_entry(q, st, &set, &entry, &elem) || !q.ps().fsets[set].any) return false;
  const size_t at = (size_t)q.ps().fsets[set].anyi * q.part->n + q.local;
  const uint32_t k = q.part->fe_akey[at];
  if (k >= FE_KEY_PASS || (k & 7u) != st) return false;
  if (rh.foreach_chain && (k >> 3) != elem) return false;
  *key = k;
  *cw = q.part->fe_acode[at];
  *set_o = set;
  *alt0 = 0;
  for (uint32_t i = 0; i < q.ps().fsets[set].anyi; i++) *alt0 += q.ps().fsets[q.ps().fanys[i]].alt_prog.size();
  return true;
}

// A FAIL / ERROR pair (status st) of a device foreach rule that a pattern entry or an anyPattern
// entry decided: the deciding set and element, from the fetched reduction keys. Unlike any_pair it
// knows the ERROR of an any set, which only the substitution gives (KV_COMPILE_FOREACH_PATVARS).
bool walked_pair(const Pair& q, uint8_t st, uint32_t* set_o, uint32_t* elem_o) {
  if (!q.part) return false;
  const RuleHost& rh = q.ps().rhost[q.rule];
  if (!rh.foreach_set && !rh.foreach_chain) return false;
  uint32_t set, entry, elem;
  if (!deciding_entry(q, st, &set, &entry, &elem)) return false;
  const FeSet& s = q.ps().fsets[set];
  uint32_t k;
  if (s.pattern && !q.part->fe_key.empty()) k = q.part->fe_key[(size_t)s.pat * q.part->n + q.local];
  else if (s.any && !q.part->fe_akey.empty()) k = q.part->fe_akey[(size_t)s.anyi * q.part->n + q.local];
  else return false;
  if (k >= FE_KEY_PASS || (k & 7u) != st) return false;
  if (rh.foreach_chain && (k >> 3) != elem) return false;
  *set_o = set;
  *elem_o = k >> 3;
  return true;
}

// Go %v of the substituted pattern value at the dynamic leaf of record e of a foreach entry's
// pattern (KV_COMPILE_FOREACH_PATVARS), on element `elem` of the pair's resource; false: not such a leaf
bool elem_pattern_value(const Pair& q, const ErrRec& e, uint32_t elem, std::string* pv) {
  const PolicySet& ps = q.ps();
  if (e.pnode >= ps.pnodes.size() || ps.pnodes[e.pnode].fe_key < 0) return false;
  const uint32_t o = foreach_elem_outcome(ps, q.kb->b, q.kb->fe_host(ps), (uint32_t)ps.pnodes[e.pnode].fe_key, q.local, elem);
  *pv = pattern_go_v(outcome_value(q.kb->b.vout_tab[o]));
  return true;
}

// alternative `alt` of an any_pair: its status on the deciding element and its record
int any_alt(const Pair& q, uint32_t alt, uint32_t* status, ErrRec8* rec) {
  uint32_t key, cw, set;
  size_t alt0;
  if (!any_pair(q, &key, &cw, &set, &alt0)) return KV_E_INVALID;
  if (alt >= q.ps().fsets[set].alt_prog.size()) return KV_E_RANGE;
  *status = (cw >> (4u * alt)) & 15u;
  if (*status != ST_FAIL && *status != ST_ERROR && *status != ST_SKIP) return KV_E_INVALID;
  *rec = q.part->fe_arec[(alt0 + alt) * q.part->n + q.local];
  return 0;
}

}  // namespace

extern "C" {

int kv_result_status(const kv_result* r, const uint8_t** status, uint64_t* n_rules, uint64_t* n_res) {
  if (!r) return KV_E_INVALID;
  if (status) {
    const int rc = guarded(KV_E_NOMEM, nullptr, [&]() -> int {
      *status = const_cast<kv_result*>(r)->status_caller();
      return 0;
    });
    if (rc) return rc;
  }
  if (n_rules) *n_rules = r->n_rules;
  if (n_res) *n_res = r->n_res;
  return 0;
}

int kv_result_phase(const kv_result* r, uint32_t i, const char** name, double* ms) {
  if (!r) return KV_E_INVALID;
  if (i >= r->phases.size()) return KV_E_RANGE;
  if (name) *name = r->phases[i].first.c_str();
  if (ms) *ms = r->phases[i].second;
  return 0;
}

int kv_result_counts(const kv_result* r, const int64_t** counts) {
  if (!r || !counts) return KV_E_INVALID;
  *counts = r->counts.data();
  return 0;
}

int kv_result_scope_counts(const kv_result* r, const int64_t** counts, uint32_t* n_scopes) {
  if (!r || !counts) return KV_E_INVALID;
  if (!(r->mode & KV_MODE_SCOPES)) return KV_E_INVALID;
  *counts = r->scope_counts.data();
  if (n_scopes) *n_scopes = (uint32_t)r->b->b.namespaces.size();
  return 0;
}

int kv_result_path(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap) {
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, true);
    if (q.code) return q.code;
    // (a deny FAIL has no failing path, as a gated SKIP)
    if (q.ps().rules[rule].deny || q.status() != ST_FAIL) return KV_E_INVALID;
    ErrRec e;
    const Batch* bt = nullptr;
    if (!q.record(&e, &bt)) return KV_E_INVALID;
    return put_message(render_path(q.ps(), *bt, e), buf, cap);
  });
}

int kv_result_error(const kv_result* r, uint32_t rule, uint64_t res, uint32_t* kind, uint32_t* flags) {
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, true);
    if (q.code) return q.code;
    ErrRec e;
    const Batch* bt = nullptr;
    if (!is_record(q.status()) || !q.record(&e, &bt)) return KV_E_INVALID;
    if (kind) *kind = e.kind_flags & 0xFFFF;
    if (flags) *flags = e.kind_flags >> 16;
    return 0;
  });
}

int kv_result_error_message(const kv_result* r, uint32_t rule, uint64_t res, const char* resource_json, size_t len,
                            char* buf, size_t cap) {
  if (!resource_json) return KV_E_INVALID;
  return guarded(KV_E_PARSE, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, true);
    if (q.code) return q.code;
    if (!is_record(q.status())) return KV_E_INVALID;
    // the caller's document of its resource `res`, the record of its status slot
    JDoc doc;
    parse_json(resource_json, len, NUM_UNSTRUCTURED, &doc);
    ErrRec e;
    const Batch* bt = nullptr;
    if (!q.record(&e, &bt)) return KV_E_INVALID;
    const PolicySet& ps = q.ps();
    std::string pv;
    const std::string* dyn_pv = nullptr;
    if (e.pnode < ps.pnodes.size() && ps.pnodes[e.pnode].dleaf >= 0) {
      const DynHost& h = q.kb->dyn_host(ps);
      const uint32_t o = h.dleaf[(size_t)ps.pnodes[e.pnode].dleaf * q.n_local() + q.local];
      pv = pattern_go_v(outcome_value(q.kb->b.vout_tab[o]));
      dyn_pv = &pv;
    }
    const std::string m = error_message(ps, *bt, e, doc, dyn_pv);
    if (m.empty()) return KV_E_INVALID;  // a compile-time constant status: no pattern error record
    return put_message(m, buf, cap);
  });
}

int kv_result_subst_error(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap) {
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, false);
    if (q.code) return q.code;
    const RuleRec& rr = q.ps().rules[rule];
    if (!rr.dyn || !q.part || q.status() != ST_ERROR) return 0;
    const DynHost& h = q.kb->dyn_host(q.ps());
    const size_t i = (size_t)(rr.dyn - 1) * q.n_local() + q.local;
    if (h.dyn_st[i] != ST_ERROR) return 0;
    // ruleError(rule, Validation, "variable substitution failed", err) (validation.go:186-188)
    return put_message("variable substitution failed: " + q.kb->b.vout_tab[h.dyn_msg[i]].substr(1), buf, cap);
  });
}

int kv_result_precond_message(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap) {
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, false);
    if (q.code) return q.code;
    const RuleRec& rr = q.ps().rules[rule];
    if (!rr.pre || !q.part || q.status() != ST_SKIP) return 0;
    // the pair recomputed from the batch's tables: a SKIP of the pattern's condition anchors has
    // another cause
    if (pre_status_host(q.kb->pre_host(q.ps()), rr.pre - 1, q.n_local(), q.local) != ST_SKIP) return 0;
    // ruleResponse(rule, Validation, "preconditions not met", RuleStatusSkip) (validation.go:183-184)
    return put_message("preconditions not met", buf, cap);
  });
}

int kv_result_deny_message(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap) {
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, false);
    if (q.code) return q.code;
    const RuleRec& rr = q.ps().rules[rule];
    if (!rr.deny || q.ps().rhost[rule].foreach_set || q.ps().rhost[rule].foreach_chain || !q.part || q.status() != ST_ERROR)
      return 0;
    // the error recomputed from the batch's outcome rows: the first unresolved string of the block
    const std::string e = deny_error_host(q.ps(), q.kb->b, rr.deny - 1, q.local);
    if (e.empty()) return 0;
    // ruleError(rule, Validation, "failed to substitute variables in deny conditions", err)
    // (validation.go:301-304)
    return put_message("failed to substitute variables in deny conditions: " + e, buf, cap);
  });
}

int kv_result_foreach_element(const kv_result* r, uint32_t rule, uint64_t res, uint32_t* index) {
  if (!index) return KV_E_INVALID;
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, false);
    if (q.code) return q.code;
    *index = 0xFFFFFFFFu;
    const uint32_t set = q.ps().rhost[rule].foreach_set;
    if (q.ps().rhost[rule].foreach_chain) {  // several entries: the chain key fetched with the statuses
      const uint8_t cst = q.status();
      uint32_t s, entry, e;
      if ((cst == ST_FAIL || cst == ST_ERROR) && deciding_entry(q, cst, &s, &entry, &e)) *index = e;
      return 0;
    }
    if (!set || !q.part) return 0;  // (not a device foreach rule: not reported)
    const uint8_t st = q.status();
    if (st != ST_FAIL && st != ST_ERROR) return 0;  // (PASS, SKIP: no deciding element)
    if (q.ps().fsets[set - 1].pattern) {  // a pattern entry: the key fetched with the statuses
      uint32_t key;
      ErrRec8 rec;
      if (pattern_pair(q, &key, &rec)) *index = key >> 3;
      return 0;
    }
    if (q.ps().fsets[set - 1].any) {  // an anyPattern entry likewise
      uint32_t key, cw, s;
      size_t a0;
      if (any_pair(q, &key, &cw, &s, &a0)) *index = key >> 3;
      else if (st == ST_ERROR && walked_pair(q, st, &s, &key)) *index = key;  // (a substitution error)
      return 0;
    }
    uint32_t e = 0xFFFFFFFFu;
    if (foreach_fold_host(q.kb->fe_host(q.ps()), set - 1, q.n_local(), q.local, &e) == st) *index = e;
    return 0;
  });
}

int kv_result_foreach_entry(const kv_result* r, uint32_t rule, uint64_t res, uint32_t* entry) {
  if (!entry) return KV_E_INVALID;
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, false);
    if (q.code) return q.code;
    *entry = 0xFFFFFFFFu;
    const RuleHost& rh = q.ps().rhost[rule];
    if (rh.foreach_set) {  // one entry: entry 0 where an element decided
      uint32_t e = 0xFFFFFFFFu;
      const int rc = kv_result_foreach_element(r, rule, res, &e);
      if (rc == 0 && e != 0xFFFFFFFFu) *entry = 0;
      return rc;
    }
    if (!rh.foreach_chain) return 0;
    const uint8_t st = q.status();
    uint32_t s, k, e;
    if ((st == ST_FAIL || st == ST_ERROR) && deciding_entry(q, st, &s, &k, &e)) *entry = k;
    return 0;
  });
}

int kv_result_foreach_message(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap) {
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, false);
    if (q.code) return q.code;
    const PolicySet& ps = q.ps();
    const uint32_t fs = ps.rhost[rule].foreach_set;
    if (ps.rhost[rule].foreach_chain) {
      // several entries: the chain key tells what the fold decided. An ERROR is the deciding deny
      // entry's first unresolved string, resolved under its leak context; a pattern entry's is its
      // element's pattern error (kv_result_foreach_error_message)
      const uint8_t cst = q.status();
      uint32_t key;
      if ((cst != ST_ERROR && cst != ST_SKIP) || !chain_key(q, &key)) return 0;
      if (cst == ST_SKIP) {
        const RuleRec& rr = ps.rules[rule];
        if (rr.pre && pre_status_host(q.kb->pre_host(ps), rr.pre - 1, q.n_local(), q.local) == ST_SKIP) return 0;
        return key == FE_KEY_NONE ? put_message("rule skipped", buf, cap) : 0;
      }
      uint32_t s, entry, e;
      if (!deciding_entry(q, cst, &s, &entry, &e) || ps.fsets[s].pattern || ps.fsets[s].any) return 0;
      const std::string err = foreach_error_host(ps, q.kb->b, q.kb->fe_host(ps), s, q.local, e);
      if (err.empty()) return 0;
      return put_message("validation failed in foreach rule for failed to substitute variables in deny conditions: " + err,
                         buf, cap);
    }
    if (!fs || !q.part) return 0;
    const uint8_t st = q.status();
    if (st != ST_ERROR && st != ST_SKIP) return 0;
    if (ps.fsets[fs - 1].pattern) {
      // a pattern entry has no host fold: an ERROR is its element's pattern error
      // (kv_result_foreach_error_message); a SKIP is "rule skipped" unless the rule's own
      // preconditions decided it, and the fetched key tells: they leave the fold's key untouched
      if (st != ST_SKIP || q.part->fe_key.empty()) return 0;
      const RuleRec& rr = ps.rules[rule];
      if (rr.pre && pre_status_host(q.kb->pre_host(ps), rr.pre - 1, q.n_local(), q.local) == ST_SKIP) return 0;
      if (q.part->fe_key[(size_t)ps.fsets[fs - 1].pat * q.part->n + q.local] != FE_KEY_NONE) return 0;
      return put_message("rule skipped", buf, cap);
    }
    if (ps.fsets[fs - 1].any) {  // an anyPattern entry likewise (it has no ERROR of its own)
      if (st != ST_SKIP || q.part->fe_akey.empty()) return 0;
      const RuleRec& rr = ps.rules[rule];
      if (rr.pre && pre_status_host(q.kb->pre_host(ps), rr.pre - 1, q.n_local(), q.local) == ST_SKIP) return 0;
      if (q.part->fe_akey[(size_t)ps.fsets[fs - 1].anyi * q.part->n + q.local] != FE_KEY_NONE) return 0;
      return put_message("rule skipped", buf, cap);
    }
    const FeHost& h = q.kb->fe_host(ps);
    uint32_t e = 0xFFFFFFFFu;
    // the pair recomputed from the batch's tables: a SKIP of the rule's own preconditions has
    // another cause (kv_result_precond_message)
    if (foreach_fold_host(h, fs - 1, q.n_local(), q.local, &e) != st) return 0;
    if (st == ST_SKIP) {
      const RuleRec& rr = ps.rules[rule];
      if (rr.pre && pre_status_host(q.kb->pre_host(ps), rr.pre - 1, q.n_local(), q.local) == ST_SKIP) return 0;
      return put_message("rule skipped", buf, cap);  // (validation.go:279-281)
    }
    const std::string err = foreach_error_host(ps, q.kb->b, h, fs - 1, q.local, e);
    if (err.empty()) return 0;
    return put_message("validation failed in foreach rule for failed to substitute variables in deny conditions: " + err,
                       buf, cap);
  });
}

int kv_result_foreach_path(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap) {
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, false);
    if (q.code) return q.code;
    uint32_t key;
    ErrRec8 rec;
    if (!pattern_pair(q, &key, &rec) || (key & 7u) != ST_FAIL) return KV_E_INVALID;
    // (the set's pattern nodes start at its own root: the path is relative to the element)
    return put_message(render_path(q.ps(), q.r->batch_of(*q.part), kv_result::decode(rec)), buf, cap);
  });
}

int kv_result_foreach_error_message(const kv_result* r, uint32_t rule, uint64_t res, const char* element_json, size_t len,
                                    char* buf, size_t cap) {
  if (!element_json) return KV_E_INVALID;
  return guarded(KV_E_PARSE, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, false);
    if (q.code) return q.code;
    uint32_t key;
    ErrRec8 rec;
    if (!pattern_pair(q, &key, &rec)) return KV_E_INVALID;
    // the element comes out of the JSON context: every number of it is float64 ('%v' 8.08e+06,
    // %T float64)
    JDoc doc;
    parse_json(element_json, len, NUM_FLOAT, &doc);
    const ErrRec e = kv_result::decode(rec);
    std::string pv;  // (a dynamic leaf: the deciding element's substituted pattern value)
    const bool dyn = elem_pattern_value(q, e, key >> 3, &pv);
    const std::string m = error_message(q.ps(), q.r->batch_of(*q.part), e, doc, dyn ? &pv : nullptr);
    if (m.empty()) return KV_E_INVALID;
    return put_message(m, buf, cap);
  });
}

int kv_result_foreach_subst_error(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap) {
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, false);
    if (q.code) return q.code;
    const PolicySet& ps = q.ps();
    const RuleHost& rh = ps.rhost[rule];
    if ((!rh.foreach_set && !rh.foreach_chain) || !(ps.n_vpats || ps.n_vanys) || !q.part) return 0;
    if (q.status() != ST_ERROR) return 0;
    uint32_t set, elem;
    if (!walked_pair(q, ST_ERROR, &set, &elem) || ps.fsets[set].vorder.empty()) return 0;
    // recomputed from the deciding element's outcome row, as kv_result_deny_message does
    const FeHost& h = q.kb->fe_host(ps);
    if (foreach_subst_host(h, set, q.n_local(), q.local, elem) != ST_ERROR) return 0;
    const std::string err = foreach_subst_error_host(ps, q.kb->b, h, set, q.local, elem);
    if (err.empty()) return 0;
    // ruleError(rule, Validation, "variable substitution failed", err) of the element's validate()
    // (validation.go:186-188), wrapped by the foreach loop (validation.go:248-252)
    return put_message("validation failed in foreach rule for variable substitution failed: " + err, buf, cap);
  });
}

int kv_rule_foreach_patvars(const kv_policyset* ps, uint32_t rule, uint32_t* on) {
  if (!ps || !on) return KV_E_INVALID;
  if (rule >= ps->ps.rules.size()) return KV_E_RANGE;
  const RuleHost& rh = ps->ps.rhost[rule];
  *on = 0;
  if (rh.foreach_set) *on = ps->ps.fsets[rh.foreach_set - 1].vorder.empty() ? 0u : 1u;
  if (rh.foreach_chain)
    for (uint32_t s : ps->ps.fe_chains[rh.foreach_chain - 1]) *on |= ps->ps.fsets[s].vorder.empty() ? 0u : 1u;
  return 0;
}

int kv_batch_foreach_subst(const kv_policyset* ps, const kv_batch* b, uint32_t set, uint64_t res, uint32_t elem,
                           uint32_t* code, char* buf, size_t cap) {
  if (!ps || !b || !code) return KV_E_INVALID;
  if (set >= ps->ps.fsets.size() || res >= b->b.res.size()) return KV_E_RANGE;
  if (ps->ps.fsets[set].vorder.empty()) return KV_E_INVALID;
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const FeHost& h = const_cast<kv_batch*>(b)->fe_host(ps->ps);
    const uint32_t* inv = const_cast<kv_batch*>(b)->inverse();
    const uint64_t s = inv ? inv[res] : res, n = b->b.res.size();
    if (elem >= b->b.fcount[s * ps->ps.flists.size() + ps->ps.fsets[set].list]) return KV_E_RANGE;
    *code = foreach_subst_host(h, set, n, s, elem);
    return put_message(*code == ST_ERROR ? foreach_subst_error_host(ps->ps, b->b, h, set, s, elem) : std::string(), buf, cap);
  });
}

int kv_result_foreach_alt(const kv_result* r, uint32_t rule, uint64_t res, uint32_t alt, uint32_t* status, char* buf,
                          size_t cap) {
  if (!status) return KV_E_INVALID;
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, false);
    if (q.code) return q.code;
    ErrRec8 rec;
    const int rc = any_alt(q, alt, status, &rec);
    if (rc) return rc;
    if (*status != ST_FAIL) return put_message(std::string(), buf, cap);
    // (the alternative's pattern nodes start at its own root: the path is relative to the element)
    return put_message(render_path(q.ps(), q.r->batch_of(*q.part), kv_result::decode(rec)), buf, cap);
  });
}

int kv_result_foreach_alt_error_message(const kv_result* r, uint32_t rule, uint64_t res, uint32_t alt,
                                        const char* element_json, size_t len, char* buf, size_t cap) {
  if (!element_json) return KV_E_INVALID;
  return guarded(KV_E_PARSE, nullptr, [&]() -> int {
    const Pair q = pair_of(r, rule, res, false);
    if (q.code) return q.code;
    uint32_t status;
    ErrRec8 rec;
    const int rc = any_alt(q, alt, &status, &rec);
    if (rc) return rc;
    JDoc doc;  // (every number of the element float64, as kv_result_foreach_error_message)
    parse_json(element_json, len, NUM_FLOAT, &doc);
    const ErrRec e = kv_result::decode(rec);
    std::string pv;  // (a dynamic leaf: the deciding element's substituted pattern value)
    uint32_t key = 0, cw, set;
    size_t alt0;
    const bool dyn = any_pair(q, &key, &cw, &set, &alt0) && elem_pattern_value(q, e, key >> 3, &pv);
    const std::string m = error_message(q.ps(), q.r->batch_of(*q.part), e, doc, dyn ? &pv : nullptr);
    if (m.empty()) return KV_E_INVALID;
    return put_message(m, buf, cap);
  });
}

int kv_policyset_deny_sets(const kv_policyset* ps, uint32_t* sets, uint32_t* conditions, uint32_t* strings) {
  if (!ps) return KV_E_INVALID;
  if (sets) *sets = (uint32_t)ps->ps.dsets.size();
  if (conditions) *conditions = (uint32_t)ps->ps.deny.conds.size();
  if (strings) *strings = (uint32_t)ps->ps.deny.keys.size();
  return 0;
}

int kv_batch_deny_fold(const kv_policyset* ps, const kv_batch* b, uint32_t set, uint8_t* status, uint64_t n) {
  if (!ps || !b || !status) return KV_E_INVALID;
  if (set >= ps->ps.dsets.size() || n != b->b.res.size()) return KV_E_RANGE;
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    CondHost h;
    build_deny(ps->ps, b->b, &h);
    const std::vector<uint32_t>& order = b->b.order;  // store index -> caller index (empty: identity)
    for (uint64_t s = 0; s < n; s++) status[order.empty() ? s : order[s]] = deny_status_host(h, set, n, s);
    return 0;
  });
}

int kv_rule_deny_set(const kv_policyset* ps, uint32_t rule, uint32_t* set) {
  if (!ps || !set) return KV_E_INVALID;
  if (rule >= ps->ps.rules.size()) return KV_E_RANGE;
  *set = ps->ps.rhost[rule].foreach_set || ps->ps.rhost[rule].foreach_chain ? 0u : ps->ps.rules[rule].deny;
  return 0;
}

// ------------------------------------------------------------------ foreach
int kv_policyset_foreach_sets(const kv_policyset* ps, uint32_t* sets, uint32_t* lists, uint32_t* conditions,
                              uint32_t* strings) {
  if (!ps) return KV_E_INVALID;
  if (sets) *sets = (uint32_t)ps->ps.fsets.size();
  if (lists) *lists = (uint32_t)ps->ps.flists.size();
  if (conditions) *conditions = (uint32_t)ps->ps.elem.conds.size();
  if (strings) *strings = (uint32_t)ps->ps.fkeys.size();
  return 0;
}

int kv_rule_foreach_set(const kv_policyset* ps, uint32_t rule, uint32_t* set) {
  if (!ps || !set) return KV_E_INVALID;
  if (rule >= ps->ps.rules.size()) return KV_E_RANGE;
  *set = ps->ps.rhost[rule].foreach_set;
  return 0;
}

int kv_rule_foreach_pattern(const kv_policyset* ps, uint32_t rule, uint32_t* on) {
  if (!ps || !on) return KV_E_INVALID;
  if (rule >= ps->ps.rules.size()) return KV_E_RANGE;
  const uint32_t fs = ps->ps.rhost[rule].foreach_set;
  *on = fs && ps->ps.fsets[fs - 1].pattern ? 1u : 0u;
  return 0;
}

int kv_batch_foreach_fold(const kv_policyset* ps, const kv_batch* b, uint32_t set, uint8_t* status, uint32_t* elem,
                          uint64_t n) {
  if (!ps || !b || !status) return KV_E_INVALID;
  if (set >= ps->ps.fsets.size() || n != b->b.res.size()) return KV_E_RANGE;
  if (ps->ps.fsets[set].pattern || ps->ps.fsets[set].any) return KV_E_INVALID;  // (no host evaluator)
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    FeHost h;
    build_foreach(ps->ps, b->b, &h);
    const std::vector<uint32_t>& order = b->b.order;  // store index -> caller index (empty: identity)
    for (uint64_t s = 0; s < n; s++) {
      uint32_t e = 0xFFFFFFFFu;
      const uint64_t i = order.empty() ? s : order[s];
      status[i] = foreach_fold_host(h, set, n, s, &e);
      if (elem) elem[i] = e;
    }
    return 0;
  });
}

int kv_policyset_foreach_chains(const kv_policyset* ps, uint32_t* chains) {
  if (!ps || !chains) return KV_E_INVALID;
  *chains = (uint32_t)ps->ps.fe_chains.size();
  return 0;
}

int kv_rule_foreach_chain(const kv_policyset* ps, uint32_t rule, uint32_t* chain_plus_1, uint32_t* n_entries) {
  if (!ps || !chain_plus_1) return KV_E_INVALID;
  if (rule >= ps->ps.rules.size()) return KV_E_RANGE;
  const uint32_t ch = ps->ps.rhost[rule].foreach_chain;
  *chain_plus_1 = ch;
  if (n_entries) *n_entries = ch ? (uint32_t)ps->ps.fe_chains[ch - 1].size() : 0u;
  return 0;
}

int kv_chain_entry_set(const kv_policyset* ps, uint32_t chain, uint32_t k, uint32_t* set) {
  if (!ps || !set) return KV_E_INVALID;
  if (chain >= ps->ps.fe_chains.size() || k >= ps->ps.fe_chains[chain].size()) return KV_E_RANGE;
  *set = ps->ps.fe_chains[chain][k];
  return 0;
}

int kv_batch_foreach_chain_fold(const kv_policyset* ps, const kv_batch* b, uint32_t chain, uint8_t* status, uint32_t* entry,
                                uint32_t* elem, uint64_t n) {
  if (!ps || !b || !status) return KV_E_INVALID;
  if (chain >= ps->ps.fe_chains.size() || n != b->b.res.size()) return KV_E_RANGE;
  for (uint32_t s : ps->ps.fe_chains[chain])
    if (ps->ps.fsets[s].pattern || ps->ps.fsets[s].any) return KV_E_INVALID;  // (no host evaluator)
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    FeHost h;
    build_foreach(ps->ps, b->b, &h);
    FeChainScratch scratch;
    const std::vector<uint32_t>& order = b->b.order;  // store index -> caller index (empty: identity)
    for (uint64_t s = 0; s < n; s++) {
      uint32_t k = 0xFFFFFFFFu, e = 0xFFFFFFFFu;
      const uint64_t i = order.empty() ? s : order[s];
      status[i] = foreach_chain_fold_host(h, chain, n, s, &k, &e, &scratch);
      if (entry) entry[i] = k;
      if (elem) elem[i] = e;
    }
    return 0;
  });
}

int kv_batch_foreach_chain_message(const kv_policyset* ps, const kv_batch* b, uint32_t chain, uint64_t res, char* buf,
                                   size_t cap) {
  if (!ps || !b) return KV_E_INVALID;
  if (chain >= ps->ps.fe_chains.size() || res >= b->b.res.size()) return KV_E_RANGE;
  for (uint32_t s : ps->ps.fe_chains[chain])
    if (ps->ps.fsets[s].pattern || ps->ps.fsets[s].any) return KV_E_INVALID;
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    const FeHost& h = const_cast<kv_batch*>(b)->fe_host(ps->ps);
    const std::vector<uint32_t>& order = b->b.order;  // store index -> caller index (empty: identity)
    uint64_t s = res;
    if (!order.empty()) s = (uint64_t)(std::find(order.begin(), order.end(), (uint32_t)res) - order.begin());
    uint32_t k = 0xFFFFFFFFu, e = 0xFFFFFFFFu;
    const uint8_t st = foreach_chain_fold_host(h, chain, b->b.res.size(), s, &k, &e);
    if (st == ST_SKIP) return put_message("rule skipped", buf, cap);  // (validation.go:279-281)
    if (st != ST_ERROR) return 0;
    const std::string err = foreach_error_host(ps->ps, b->b, h, ps->ps.fe_chains[chain][k], s, e);
    if (err.empty()) return 0;
    return put_message("validation failed in foreach rule for failed to substitute variables in deny conditions: " + err,
                       buf, cap);
  });
}

int kv_batch_foreach_tables(const kv_policyset* ps, const kv_batch* b, char** out, size_t* len) {
  if (!ps || !b || !out || !len) return KV_E_INVALID;
  return guarded(KV_E_INVALID, nullptr, [&]() -> int {
    FeHost h;
    build_foreach(ps->ps, b->b, &h);
    std::string o;
    auto put = [&](const std::vector<uint32_t>& v) {
      const uint64_t n = v.size();
      o.append((const char*)&n, 8);
      o.append((const char*)v.data(), n * 4);
    };
    for (const std::vector<uint32_t>* v :
         {&h.sets, &h.lists, &h.el_res, &h.el_ord, &h.lstate, &h.first, &h.pats, &h.chain, &h.chains, &h.chain_ents,
          &h.anys, &h.any_alts,
          &h.gate.sets, &h.gate.ents, &h.deny.sets, &h.deny.ents, &h.deny.outc, &h.deny.truth, &h.deny.unk, &h.deny.err,
          &h.deny.oos})
      put(*v);
    put({h.deny.words, h.max_el});
    if (h.has_vars())  // (KV_COMPILE_FOREACH_PATVARS: nothing is added without a set with variable strings)
      for (const std::vector<uint32_t>* v : {&h.vruns, &h.vrows, &h.mpl}) put(*v);
    char* p = (char*)malloc(std::max<size_t>(o.size(), 1));
    if (!p) return KV_E_NOMEM;
    memcpy(p, o.data(), o.size());
    *out = p;
    *len = o.size();
    return 0;
  });
}

int kv_rule_foreach_anypattern(const kv_policyset* ps, uint32_t rule, uint32_t* n_alts) {
  if (!ps || !n_alts) return KV_E_INVALID;
  if (rule >= ps->ps.rules.size()) return KV_E_RANGE;
  const uint32_t fs = ps->ps.rhost[rule].foreach_set;
  *n_alts = fs && ps->ps.fsets[fs - 1].any ? (uint32_t)ps->ps.fsets[fs - 1].alt_prog.size() : 0u;
  return 0;
}

int kv_foreach_set_alternatives(const kv_policyset* ps, uint32_t set, uint32_t* n) {
  if (!ps || !n) return KV_E_INVALID;
  if (set >= ps->ps.fsets.size()) return KV_E_RANGE;
  *n = ps->ps.fsets[set].any ? (uint32_t)ps->ps.fsets[set].alt_prog.size() : 0u;
  return 0;
}

int kv_foreach_set_pattern(const kv_policyset* ps, uint32_t set, uint32_t* on) {
  if (!ps || !on) return KV_E_INVALID;
  if (set >= ps->ps.fsets.size()) return KV_E_RANGE;
  *on = ps->ps.fsets[set].pattern ? 1u : 0u;
  return 0;
}

int kv_policyset_cond_sets(const kv_policyset* ps, uint32_t* sets, uint32_t* conditions, uint32_t* strings) {
  if (!ps) return KV_E_INVALID;
  if (sets) *sets = (uint32_t)ps->ps.csets.size();
  if (conditions) *conditions = (uint32_t)ps->ps.gate.conds.size();
  if (strings) *strings = (uint32_t)ps->ps.gate.keys.size();
  return 0;
}

double kv_result_kernel_ms(const kv_result* r) { return r ? r->kernel_ms : -1.0; }

int kv_result_failures(const kv_result* cr, uint64_t* n, const uint32_t** rule, const uint64_t** res,
                       const uint32_t** path_id) {
  if (!cr || !cr->has_err() || !n) return KV_E_INVALID;
  kv_result* r = const_cast<kv_result*>(cr);
  const int rc = guarded(KV_E_NOMEM, nullptr, [&]() -> int {
    std::call_once(r->fail_once, [r]() {
      // one pass over the statuses: records come rule-major, in resource order per part
      std::unordered_map<uint64_t, uint32_t> compact;      // (path pnode, packed indices) -> path id
      std::unordered_map<std::string, uint32_t> rendered;  // wide records: by rendered path
      const PolicySet& ps = *r->ps;
      const uint8_t* stm = r->st_store();
      for (uint32_t rl = 0; rl < r->n_rules; rl++) {
        const uint8_t* row = stm + (size_t)rl * r->n_res;
        for (const ResultPart& p : r->parts) {
          uint64_t i = p.base[rl];
          for (uint64_t q = p.lo; q < p.lo + p.n; q++) {
            const uint8_t st = row[q];
            if (!is_record(st)) continue;
            uint32_t id = KV_PATH_NONE;
            if (st == ST_FAIL && !ps.rules[rl].deny) {  // (a deny FAIL has an empty record: no failing path)
              const ErrRec8 c = p.r8(rl, i);
              if ((c.w0 & ERR8_WIDE) && !p.recw.empty()) {
                const std::string path = render_path(ps, r->batch_of(p), p.recw[i]);
                auto it = rendered.find(path);
                if (it == rendered.end()) {
                  it = rendered.emplace(path, (uint32_t)r->f_paths.size()).first;
                  r->f_paths.push_back(path);
                }
                id = it->second;
              } else {
                const ErrRec e = kv_result::decode(c);
                const uint64_t key = (uint64_t)path_pnode(ps, e) << 32 | (c.w1 & ERR8_IDX_MASK);
                auto it = compact.find(key);
                if (it == compact.end()) {
                  const std::string path = render_path(ps, r->batch_of(p), e);
                  auto jt = rendered.find(path);
                  if (jt == rendered.end()) {
                    jt = rendered.emplace(path, (uint32_t)r->f_paths.size()).first;
                    r->f_paths.push_back(path);
                  }
                  it = compact.emplace(key, jt->second).first;
                }
                id = it->second;
              }
            }
            r->f_rule.push_back(rl);
            r->f_res.push_back(r->cidx(q));
            r->f_path.push_back(id);
            i++;
          }
        }
      }
      if (!r->b->b.order.empty() && !r->caller_order) {
        // caller order: by rule, then caller resource index. Each rule's pairs are a subset of
        // [0, n_res) with distinct caller indices: a rule with pairs on 1/16 of the resources or more
        // is scattered into a per-thread slot array and swept in order, a sparser one sorted
        // (rules split over host threads)
        std::vector<size_t> rb(r->n_rules + 1, 0);
        for (size_t i = 0; i < r->f_rule.size(); i++) rb[r->f_rule[i] + 1]++;
        for (uint32_t rl = 0; rl < r->n_rules; rl++) rb[rl + 1] += rb[rl];
        std::vector<uint64_t> fs(r->f_res.size());
        std::vector<uint32_t> fp(r->f_path.size());
        const unsigned T = kv_result::host_threads();
        std::vector<std::thread> th;
        for (unsigned t = 0; t < T; t++)
          th.emplace_back([&, t]() {
            // caller index -> path id + 1 (0: no pair; 64-bit: KV_PATH_NONE + 1 of an ERROR / SKIP
            // pair must not wrap to "no pair")
            std::vector<uint64_t> slot;
            for (uint32_t rl = t; rl < r->n_rules; rl += T) {
              if (rb[rl] == rb[rl + 1]) continue;
              if ((rb[rl + 1] - rb[rl]) * 16u < r->n_res) {
                std::vector<std::pair<uint64_t, uint32_t>> v;
                v.reserve(rb[rl + 1] - rb[rl]);
                for (size_t i = rb[rl]; i < rb[rl + 1]; i++) v.push_back({r->f_res[i], r->f_path[i]});
                std::sort(v.begin(), v.end());
                for (size_t i = 0; i < v.size(); i++) {
                  fs[rb[rl] + i] = v[i].first;
                  fp[rb[rl] + i] = v[i].second;
                }
                continue;
              }
              if (slot.empty()) slot.assign(r->n_res, 0ull);
              for (size_t i = rb[rl]; i < rb[rl + 1]; i++) slot[r->f_res[i]] = (uint64_t)r->f_path[i] + 1ull;
              size_t o = rb[rl];
              for (uint64_t j = 0; j < r->n_res && o < rb[rl + 1]; j++)
                if (slot[j]) {
                  fs[o] = j;
                  fp[o++] = (uint32_t)(slot[j] - 1ull);
                  slot[j] = 0ull;
                }
            }
          });
        for (auto& x : th) x.join();
        r->f_res.swap(fs);
        r->f_path.swap(fp);
        // path ids numbered by first appearance in the returned order
        std::vector<uint32_t> renum(r->f_paths.size(), KV_PATH_NONE);
        std::vector<std::string> paths;
        for (uint32_t& id : r->f_path) {
          if (id == KV_PATH_NONE) continue;
          if (renum[id] == KV_PATH_NONE) {
            renum[id] = (uint32_t)paths.size();
            paths.push_back(std::move(r->f_paths[id]));
          }
          id = renum[id];
        }
        r->f_paths.swap(paths);
      }
    });
    return 0;
  });
  if (rc) return rc;
  *n = r->f_rule.size();
  if (rule) *rule = r->f_rule.data();
  if (res) *res = r->f_res.data();
  if (path_id) *path_id = r->f_path.data();
  return 0;
}

const char* kv_path_string(const kv_result* r, uint32_t path_id) {
  if (!r || path_id >= r->f_paths.size()) return nullptr;
  return r->f_paths[path_id].c_str();
}

}  // extern "C"
