// validate.foreach on the device (kvcond.h): the list states, the per-element verdict and the
// reduction keys, shared by kv_foreach_elem_kernel / kv_foreach_pat_kernel / kv_foreach_any_kernel /
// kv_foreach_fin_kernel / kv_foreach_chain_kernel (kvkernel.hip) and the host fold (kvcond.cpp foreach_fold_host). Plain code over the tables of
// kvcond.h FeHost; needs kv_layout.h and kvblocks.h.
#pragma once

namespace kv {

// state of one (resource, foreach list)
constexpr uint8_t FE_LIST_EMPTY = 0;  // the list query is NotFound: no element
constexpr uint8_t FE_LIST_OK = 1;     // a list of maps (or one map), no null inside
constexpr uint8_t FE_LIST_OOS = 2;    // anything else: the pair is ST_CPU
constexpr uint32_t FE_MAX_ELEMS = 0x10000u;
constexpr uint32_t FE_MAX_ENTRIES = 16u;  // entries of one rule (KV_COMPILE_FOREACH_ENTRIES)
constexpr uint32_t FE_MAX_ALTS = 8u;      // alternatives of one anyPattern entry (KV_COMPILE_FOREACH_ANYPATTERN)

// Reduction keys of fe_acc[set][res] (atomicMin): the first decisive element of the resource's
// list, (index in the list << 3 | its ST_ code), below the key of "some element passed", below
// the initial value "no element, or every element skipped".
constexpr uint32_t FE_KEY_PASS = 0x80000000u;
constexpr uint32_t FE_KEY_NONE = 0xFFFFFFFFu;

// The device view of FeHost (32-bit words throughout). Row s of gate / deny is foreach set s; the
// two share outc and the truth / unknown planes, and their string rows are columns of the set's list.
struct FeTables {
  const uint32_t* sets;    // 4 words per foreach set: list, has_pre, 1 + pattern set, 1 + any set (both 0: a deny block)
  const uint32_t* lists;   // 4 words per list: first word of its outc block, elements, first plane row, first element
  CondBlocks gate;         // the entry preconditions of every set (preconditions resolver: no err / oos)
  CondBlocks deny;         // the deny block of every set; outc: per list a block [string of the list][element
                           // of the list]; err / oos: [plane row of the list + string][words]
  const uint32_t* el_res;  // per list block: the element's store resource
  const uint32_t* el_ord;  // per list block: the element's index in its list
  const uint32_t* lstate;  // [list][res]: FE_LIST_*
  uint32_t n_sets, n_lists, max_el;
  // rules of several entries (KV_COMPILE_FOREACH_ENTRIES): a chain is the ordered list of its
  // entries' foreach sets
  const uint32_t* chains;      // 2 words per chain: first entry in chain_ents, entries
  const uint32_t* chain_ents;  // one foreach set per entry
  uint32_t n_chains;
};

// Pattern sets (KV_COMPILE_FOREACH_PATTERN, kvwalk.h): the foreach sets whose entry carries a
// `pattern`. A lane finds its element's node from the resource's root along the list's path.
constexpr uint32_t FE_STEP_SLOT = 0;   // a field: the slot of the key in the map's slot list
constexpr uint32_t FE_STEP_INDEX = 1;  // an index (a negative one counts from the end)
constexpr uint32_t FE_STEP_SCAN = 2;   // a field of a keep-all map: the key id
struct FePatTables {
  const uint32_t* pats;   // 4 words per pattern set: foreach set, first instruction, first step, steps
  const uint32_t* chain;  // 2 words per step of a list path: FE_STEP_*, slot | index | key id
  const uint32_t* first;  // [list][res]: the resource's first element in the list's block
  uint32_t n_pats;
};

// Any sets (KV_COMPILE_FOREACH_ANYPATTERN): the foreach sets whose entry carries an `anyPattern`,
// the alternatives plain pattern programs tried in order per element (kv_foreach_any_kernel).
// The code word of an element: 4 bits per alternative, alternative k's ST_ status (FAIL, ERROR or
// SKIP) in bits [4k, 4k + 4), 0 for one that was not evaluated or passed. The record alone cannot
// tell ERROR from FAIL, so the status is kept beside it.
struct FeAnyTables {
  const uint32_t* anys;   // 8 words per any set: foreach set, first alternative, alternatives, first step, steps, 0, 0, 0
  const uint32_t* alts;   // per alternative: the first instruction of its program
  const uint32_t* chain;  // FePatTables::chain
  const uint32_t* first;  // FePatTables::first
  uint32_t n_anys, n_alts;
};

// Pattern variables in entries (KV_COMPILE_FOREACH_PATVARS): the pattern sets and any sets whose
// patterns hold `{{element...}}` / `{{request.object...}}` strings. The strings are strict string
// rows of the set's list (FeTables::deny: outc, err, oos), resolved per element at ingest like the
// deny strings; a dynamic leaf of the pattern program (OP_VLEAF) names its string's row in the
// list, and the predicate it evaluates is the element's outcome id in the batch predicate table
// (DevBatch::dps). Such sets stand behind the others in FePatTables::pats / FeAnyTables::anys and
// run in kernels of their own (kv_foreach_patv_kernel, kv_foreach_anyv_kernel).
struct FeVarTables {
  const uint32_t* runs;  // 2 words per set (this launch's first set at 0): first row in `rows`, rows
  const uint32_t* rows;  // the strings of a set in the substitution's traversal order (for an any set:
                         // alternative 0's, then alternative 1's, ...): the string's row in its list
  const uint32_t* mpl;   // [plane row of the list + string][words], beside err / oos: the outcome is a map or an array
  const uint32_t* ityp;  // [words], by outcome id: the outcome's predicate compares a number's text form
};

// substitutePatterns() of one element (validation.go:549-571): element e of the list L (its 4
// words of FeTables::lists) under the strings rows[r0, r0 + rn) of a set. 0: every string resolved
// to a leaf value; ST_ERROR / ST_CPU: the first string in traversal order whose outcome is an
// error / outside the resolver's scope decides; otherwise ST_CPU where a map or an array replaces
// a leaf. The run is the same for every lane of a launch row; a lane loads outc[row][e], coalesced.
KV_HD inline uint32_t kv_fe_subst(const FeTables& T, const FeVarTables& V, const uint32_t* L, uint32_t r0, uint32_t rn,
                                  uint32_t e) {
  const uint32_t* outc = T.deny.outc + L[0];
  const uint32_t n_el = L[1], W = T.deny.words;
  uint32_t structural = 0;
  for (uint32_t k = 0; k < rn; k++) {
    const uint32_t row = V.rows[r0 + k];
    const uint32_t o = outc[(uint64_t)row * n_el + e];
    const uint64_t w = (uint64_t)(L[2] + row) * W + (o >> 5);
    const uint32_t bit = 1u << (o & 31u);
    if (T.deny.err[w] & bit) return ST_ERROR;
    if (T.deny.oos[w] & bit) return ST_CPU;
    structural |= V.mpl[w] & bit;
  }
  return structural ? (uint32_t)ST_CPU : 0u;
}

// One element of foreach set `set`: element e of the set's list (e < its element count).
// validate() on the element's context (validation.go:156-202): the entry's preconditions under
// the preconditions resolver (not met: ST_SKIP, undecided: ST_CPU), then the deny block under the
// strict one (kv_deny_status: ST_CPU, ST_ERROR, ST_FAIL or ST_PASS).
KV_HD inline uint32_t kv_foreach_elem(const FeTables& T, uint32_t set, uint32_t e) {
  const uint32_t* L = T.lists + 4u * T.sets[4u * set];
  const uint32_t n_el = L[1];
  if (T.sets[4u * set + 1u]) {
    CondBlocks G = T.gate;
    G.outc += L[0];
    const uint32_t g = kv_gate_status(kv_cond_fold<false>(G, set, n_el, e));
    if (g) return g;
  }
  const uint64_t row = (uint64_t)L[2] * T.deny.words;
  CondBlocks D = T.deny;
  D.outc += L[0];
  D.err += row;
  D.oos += row;
  return kv_deny_status(kv_cond_fold<true>(D, set, n_el, e));
}

KV_HD inline bool kv_fe_decisive(uint32_t code) { return code == ST_FAIL || code == ST_ERROR || code == ST_CPU; }

// the key of one element on its own (the host fold takes the minimum over a resource's elements)
KV_HD inline uint32_t kv_fe_key(uint32_t code, uint32_t ord) {
  return kv_fe_decisive(code) ? (ord << 3 | code) : code == ST_PASS ? FE_KEY_PASS : FE_KEY_NONE;
}

// the status byte of (set, resource) from the list state and the reduced key
KV_HD inline uint32_t kv_fe_final(uint32_t lstate, uint32_t key) {
  if (lstate == FE_LIST_OOS) return ST_CPU;
  if (key == FE_KEY_NONE) return ST_SKIP;  // no element, or every element skipped: "rule skipped"
  if (key == FE_KEY_PASS) return ST_PASS;  // applyCount > 0: "rule passed"
  return key & 7u;
}

// One (chain, resource): validateForEach over the entries in order (validation.go:204-262), from
// the rows the entry sets' reduction left: per entry the state of its list on the resource and
// its key fe_acc[set][res]. An out-of-scope list ends the walk with ST_CPU; the first entry with a
// decisive element ends it with that element's code; a passing entry counts (applyCount runs
// across the entries). Without either: ST_PASS when an entry passed, else ST_SKIP. *ckey: the
// chain key, (entry << 19 | index in the entry's list << 3 | code) of the deciding pair (an
// out-of-scope list: index 0), below FE_KEY_PASS, below FE_KEY_NONE. The entry count and the
// entries' sets are the same for every lane of a launch row: the loop is uniform up to a lane's
// early exit, and each step costs the lane one word of lstate and one of fe_acc, both coalesced.
KV_HD inline uint32_t kv_fe_chain(const FeTables& T, uint32_t chain, uint64_t n_res, uint64_t r, const uint32_t* fe_acc,
                                  uint32_t* ckey) {
  const uint32_t e0 = T.chains[2u * chain], n_ent = T.chains[2u * chain + 1u];
  bool passed = false;
  for (uint32_t k = 0; k < n_ent; k++) {
    const uint32_t s = T.chain_ents[e0 + k];
    if (T.lstate[(uint64_t)T.sets[4u * s] * n_res + r] == FE_LIST_OOS) {
      *ckey = k << 19 | ST_CPU;
      return ST_CPU;
    }
    const uint32_t key = fe_acc[(uint64_t)s * n_res + r];
    if (key < FE_KEY_PASS) {
      *ckey = k << 19 | key;
      return key & 7u;
    }
    passed |= key == FE_KEY_PASS;
  }
  *ckey = passed ? FE_KEY_PASS : FE_KEY_NONE;
  return passed ? ST_PASS : ST_SKIP;
}

}  // namespace kv
