// Device-side views of a compiled policy set and an ingested batch, shared by
// the HIP kernels (kvkernel.hip, generated kernels of kvjit.cpp) and the host
// runtime (kvapi.cpp). Plain structs, no includes (embedded in the hiprtc prelude).
#pragma once

namespace kv {

struct ErrRec {
  uint32_t kind_flags;  // kind | flags << 16
  uint32_t pnode;
  uint32_t keynode;
  uint32_t resnode;
  uint32_t idx[4];
};

// Compact error record (8 B per FAIL / ERROR / SKIP pair, the one written per pass):
//   w0 = kind | flags << 4 | wide << 6 | pnode << 7          (pnode < 2^25)
//   w1 = idx0 | idx1 << 10 | idx2 << 18 | lane << 26  (idx0 < 1024, idx1 / idx2 < 256, idx3 == 0;
//        lane = the resource's lane in its wave)
// A record that does not fit (larger loop indices, a fourth loop level, a resolved
// wildcard key) sets `wide`; the host then re-runs the pass with full records
// (DevOut::full bit 2) into the 32 B ErrRec array.
// Layout in err8[rule][res]: the bytecode engine writes a record at its pair's slot; the
// specialized kernels append the records of a wave to the front of the wave's 64-slot segment
// (err8[rule][wave first resource + k], k in order of writing), so a wave writes whole lines
// instead of 8 B into 32 B sectors; the fetch restores resource order from the lane field
// (kv_rec_scatter_kernel).
struct ErrRec8 {
  uint32_t w0, w1;
};
constexpr uint32_t ERR8_WIDE = 1u << 6;
constexpr uint32_t ERR8_IDX_MASK = (1u << 26) - 1u;  // w1 without the lane

struct DevPS {
  const Inst* prog;
  const Pred* preds;
  const Alt* alts;
  const Conj* conjs;
  const Atom* atoms;
  const RuleRec* rules;
  const MFilter* filters;
  const uint32_t* fflags;  // per-filter flags folded with the launch's admission info
  const KindSpec* kinds;
  const StrRef* strrefs;
  const StrPair* strpairs;
  const Selector* sels;
  const SelLabel* sellabels;
  const SelExpr* selexprs;
  const uint32_t* kg_specs;
  const GSeg* gsegs;
  const GWord* gwords;
  const uint8_t* pstr;
  uint32_t star_id;
  uint32_t n_rules;
  uint32_t n_filters, n_sels;
  // value-predicate table of the specialized kernels (per launch configuration):
  // ptab[word * n_vals + val] bit b = leaf predicate of memo slot 32*word+b on
  // the scalar Val `val`, and on the three pseudo values after the batch's values: a
  // null, a map and an array node (n_vals = values + KV_PTAB_PSEUDO; built each pass by
  // kvj_ptab before the rule kernels)
  const uint32_t* ptab;
  uint32_t n_vals;
  // match tables (per launch configuration, built each pass by kv_mtab before the rule
  // kernels): bit b of word w at [w * n_entities + e] = filter criterion b on entity e
  //   mt_ns  [nss_bit]  namespace globs   x distinct checkNameSpace strings (DevBatch::nsms)
  //   mt_ann [ann_bit]  annotation globs  x distinct annotation lists       (DevBatch::asets)
  //   mt_sel [sel]      label selectors   x distinct label lists            (DevBatch::lsets)
  uint32_t mt_ns_words, mt_ann_words, mt_sel_words;
  const uint32_t* mt_ns;
  const uint32_t* mt_ann;
  const uint32_t* mt_sel;
  // match bits of the specialized kernels per match tuple (Res::tup): mtup[w * n_tup + tup]
  // bit b = rule at bit position 32*w+b (kernel order, kvjit.cpp) matches the tuple's
  // resources (1 for rules with name filters: evaluated per resource); built each pass by
  // kv_mfac + kv_mtup after kv_mtab (factored match, below)
  const uint32_t* mtup;
  uint32_t mtup_words;
  // filter of each namespace-glob bit (mt_ns_words * 32 entries), then of each annotation bit
  // (mt_ann_words * 32); KV_SENT for unused bits (mtab_bit_filters, kvfold.cpp)
  const uint32_t* mt_bitf;
  // Factored match (kv_mfac + kv_mtup, kvkernel.hip). MatchesResourceDescription of one
  // filter is a conjunction of per-attribute criteria (pkg/engine/utils.go:265-336), so a
  // rule's match is an OR of "planes" (one per `any` filter; `all` filters AND into one
  // plane), each the AND of five per-entity words: kind entity, checkNameSpace string,
  // annotation list, label list, namespace (namespaceSelector). A *slot* is one plane of one
  // 32-rule word (bit b = rule at bit position 32*w+b); per slot and bit, fac_bit holds the
  // plane's filter list (first, count | KV_FAC_PRESENT) in fac_flist.
  //   fac_word[4w..4w+3] = first slot of word w, match planes | exclude planes << 8,
  //                        bits evaluated per resource (name filters), bits evaluated per
  //                        tuple by rule_matches (rules with more planes than KV_FAC_MAXP)
  //   fac_rule[32w+b]    = rule at bit position 32w+b (KV_SENT: padding)
  // Tables (built each pass by kv_mfac after kv_mtab): fac_tab + fac_off[t], [slot][entity]
  // for entity type t (KV_FAC_KIND .. KV_FAC_NS).
  const uint32_t* fac_word;
  const uint32_t* fac_bit;
  const uint32_t* fac_flist;
  const uint32_t* fac_rule;
  uint32_t fac_slots, fac_words;
  uint32_t* fac_tab;
  uint64_t fac_off[5];
};
constexpr uint32_t KV_FAC_PRESENT = 0x80000000u;
constexpr uint32_t KV_FAC_MAXP = 8;  // match (and exclude) planes per word factored; beyond: rule_matches
enum FacType : uint32_t { KV_FAC_KIND = 0, KV_FAC_NSM = 1, KV_FAC_ANN = 2, KV_FAC_SEL = 3, KV_FAC_NS = 4, KV_FAC_TYPES = 5 };

struct DevBatch {
  const Node* nodes;
  const Val* vals;
  const Res* res;
  const KV* kvs;
  const uint8_t* bstr;
  const uint32_t* ns_bits;
  const uint32_t* key_off;
  const uint32_t* key_len;
  const uint8_t* kstr;
  const StrRef* nsms;   // distinct checkNameSpace strings (bstr offsets)
  const KVSet* lsets;   // distinct label lists
  const KVSet* asets;   // distinct annotation lists
  uint32_t n_nsm, n_lsets, n_asets;
  uint32_t ns_words;
  uint32_t n_res;
  const uint32_t* tup_rep;  // a resource of each match tuple (its Res is the tuple's inputs)
  uint32_t n_tup;
  // kind entities: distinct (kind, group, version, kind flags) of the batch's tuples
  const uint32_t* tup_kent;  // kind entity of each tuple
  const uint32_t* kent_rep;  // a resource of each kind entity
  uint32_t n_kent, n_ns;     // kind entities, namespaces (rows of ns_bits)
  // pattern variables (kvvars.cpp build_dyn): predicate table of the batch's distinct
  // substituted leaves, outcome (= predicate) id per [dynamic leaf][res], and the status
  // substitution decides per [dynamic rule][res] (0: evaluate, ST_ERROR, ST_CPU)
  const DevPS* dps;
  const uint32_t* dleaf;
  const uint8_t* dyn_st;
  // path columns of the specialized kernels (kvcol.h; null without them): one pool of 32-bit
  // words, every row of a family laid out by cell format (below), so a lookup loads only the
  // words its consumers read (4 bytes for a narrow cell, 12 or 16 for a wide one)
  const uint32_t* pcol;
  // condition blocks (kvcond.h, kvblocks.h; their tables go to the kernels below by value):
  // the gate kv_precond_kernel writes once per batch, pre_st[set * n_res + res] = 0 (evaluate the
  // pattern), ST_SKIP ("preconditions not met") or ST_CPU (undecided on the device)
  const uint8_t* pre_st;
  // validate.deny / validate.foreach on the device: the plane kv_deny_kernel (rows of the deny sets)
  // and kv_foreach_fin_kernel (rows of the foreach sets, after them) write once per batch,
  // deny_st[set * n_res + res] = ST_PASS, ST_FAIL, ST_ERROR, ST_CPU or (foreach) ST_SKIP, the final
  // status of the rule's pair that match / exclude and the preconditions let through
  const uint8_t* deny_st;
};

// ------------------------------------------------------------------ path columns
// The specialized kernels read every lookup whose path from the resource root (or from the
// element of a fused array loop) is static from a column of the batch's nodes at that path,
// one coalesced load, instead of chasing the path through the node rows (kvjit.cpp hoist).
// Columns come in families: family 0 has one column per root path, one row per wave group;
// family f > 0 belongs to one array path (its "family array", a column of family 0) and holds
// one column per path relative to that array's elements, one row per element with the element
// rows of each wave group together (element i of a lane's array: the row at word E + i x the
// family's row words, E = the family array cell's `c`).
// A column's cell format is chosen by the generator from what the kernels read of it (kvjit.cpp
// col_plan): a *narrow* cell is one word, 0 for an absent node, else (8 | type) << 28 | the
// Val id of a scalar (0 for null / map / array) - presence, type and value are all its
// consumers read; a *wide* cell is the present node as {type | KV_COL_PRESENT, a, c'} with c' =
// the node's own index for a map, the word offset of its element rows for a family array, the
// node's c otherwise (absent: all zero), and its b in a plane of its own when a consumer reads
// it. A row of a family with nw wide columns, nb of them with a b plane, and nn narrow ones:
//   [wide (kt, a, c) x nw x 64 lanes][b x nb x 64][narrow x nn x 64]     (32-bit words)
// A family may be *nested*: its array is a column of another element family (its parent, itself
// a family of a root-path array), and it holds one row per element of that array, the rows of
// one parent row (one wave group's element j) together: as many as the longest such array among
// the row's 64 lanes. The parent's array cell carries their word offset in `c`, the same for
// every lane of the row, so the nested cells load coalesced as the element cells do. Two levels
// only: a nested family has no nested family of its own.
// Built once per batch and device (kvcol.h, kv_pcol_* in kvkernel.hip).
constexpr uint32_t KV_COL_MAXD = 12;            // steps of a column path
constexpr uint32_t KV_COL_SCAN = 0x80000000u;   // step: key id of a keep-all map (else a slot)
constexpr uint32_t KV_COL_PRESENT = 16u;        // kt of a present cell: type | KV_COL_PRESENT
constexpr uint32_t KV_COL_PAYLOAD = 28u;        // payload bits of a narrow cell (Val ids below 2^28)
enum ColFmt : uint32_t { KV_COLF_WIDE = 0, KV_COLF_WIDEB = 1, KV_COLF_NARROW = 2 };
struct ColDesc {
  uint32_t fam;      // 0: a root path, f > 0: a path relative to the elements of family f
  uint32_t j;        // column within its family (order of first use)
  uint32_t nsteps;   // path length
  uint32_t arr_fam;  // the family whose array this column holds (0: none)
  uint32_t fmt;      // ColFmt
  uint32_t pos;      // position among the family's wide (or narrow) columns
  uint32_t bpos;     // KV_COLF_WIDEB: position in the b plane
  uint32_t steps[KV_COL_MAXD];
};
// per family: its array's column (an index into the plan's columns: a column of family 0, or of
// the parent family of a nested one; family 0: unused), its parent family (0: the array is a
// root path), its columns by format; set per batch: the first word of its element rows in the
// pool, and (device pointer) the exclusive prefix of element rows per wave group (n_groups + 1
// entries: the last one is the family's row count)
struct ColFam {
  uint32_t arr_col, ncols;
  uint32_t parent;
  uint32_t nw, nb, nn;
  uint32_t off_lo, off_hi;
  uint32_t* erow;
};

struct DevOut {
  uint8_t* status;             // [rule][res]
  ErrRec8* err8;               // [rule][res] (written for fail/error/skip)
  ErrRec* err;                 // [rule][res] (only records flagged ERR8_WIDE)
  unsigned long long* counts;  // [rule][8]
  uint32_t full;               // bit0 status, bit1 error records, bit2 full 32 B records (not 8 B),
                               // bit3 per-scope counts (specialized kernels: counted in the pass)
  unsigned long long* scounts; // [scope][rule][8] (bit3)
  const uint32_t* scope;       // scope of every resource (bit3)
  // site records of the specialized rule groups (bit1, below; null without such groups)
  uint32_t* gsite;             // 16 B records, [group area][wave][64 x members]
  uint32_t* gcnt;              // [group][wave] records written
  // specialized kernels (bit0): 1 = the workgroup's 256 statuses of the rule were written, 0 = all
  // NOMATCH and not written (kv_end_flush; the fetch fills them, kv_status_fill_kernel)
  uint8_t* sflag;              // [rule][workgroup]
};

// Site records (specialized kernels, rule groups of 2+ members; kvdevfn.h kv_gfin): the members a
// lane ends at one error site share the site's record but for their pattern nodes (the group's
// representative's node + the member's shift), so the kernel writes one 16 B record per (lane,
// site) - {kind | flags << 4 | pn << 8 of the representative (0: none), ErrRec8::w1, member mask,
// indices do not fit} - appended to the wave's segment of the group's area (64 x members slots per
// wave: a member ends once per lane), and the count per (group, wave) when the wave ends. At fetch
// kv_gsite_expand_kernel writes each member's ErrRec8 to its [rule][res] slot. Group g's area
// starts at record gpre * 64 * waves (gpre = members of the groups before it); its members are
// gs_mem[2 * (moff + j)] (rule) and [2 * (moff + j) + 1] (pattern-node shift).
struct GSiteDesc {
  uint32_t n, gpre, moff, pad;
};

constexpr int KV_WG = 256;
// Workgroup of the specialized rule kernels: four waves, 256 resources. A workgroup's statuses
// of a rule are one 256-byte row of its LDS, which the end-of-kernel flush (kvdevfn.h
// kv_end_flush) copies in 16 B pieces and counts across the waves, and one segment of the status
// matrix (DevOut::sflag, KV_WG). The waves meet at the flush's entry barrier: a wave that ends its
// blocks early holds its slot until the slowest of the four arrives.
constexpr int KV_RWG = 256;
constexpr uint32_t KV_RWAVES = (uint32_t)KV_RWG / 64u;
// LDS of a specialized rule kernel: the waves' record counters (a byte per (wave, row), wave
// stride KV_KROWS), then one status row per rule of the kernel (KV_RSTRIDE bytes: a byte per lane)
constexpr uint32_t KV_RSTRIDE = KV_RWG;
constexpr uint32_t KV_KROWS = 128u;                  // most rules (rows) per specialized kernel
constexpr uint32_t KV_ROW0 = KV_RWAVES * KV_KROWS;   // byte offset of row 0
constexpr uint32_t KV_PTAB_PSEUDO = 3;  // ptab columns of a null, a map and an array node
constexpr int KV_HIST = 8;

}  // namespace kv
