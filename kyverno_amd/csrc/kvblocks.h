// Condition blocks on the device (kvcond.h): the one table form and the one per-lane fold behind
// the precondition gate, validate.deny and the two blocks of a validate.foreach entry. Shared by
// kv_precond_kernel / kv_deny_kernel / kv_foreach_elem_kernel (kvkernel.hip), the host
// (kvcond.cpp) and the host harness tools/kvemu. Plain code; needs kv_layout.h.
#pragma once

namespace kv {

constexpr uint32_t KV_ENT_ALL = 0x80000000u;     // entry word 1: the condition is a member of `all`
constexpr uint32_t KV_ENT_NOCOND = 0x7FFFFFFFu;  // entry word 1: the string has no condition to evaluate
constexpr uint32_t KV_SET_ANY = 1u;              // set word 2: an `any` list is present
constexpr uint32_t KV_SET_FALSE = 2u;            // set word 2: a constant condition makes the block false

// The device view of kvcond.h CondHost (32-bit words throughout).
struct CondBlocks {
  const uint32_t* sets;   // 4 words per set: first entry, entries, KV_SET_* flags, 0
  const uint32_t* ents;   // 2 words per entry: string row, condition | KV_ENT_ALL or KV_ENT_NOCOND; a set's
                          // entries are ordered by string across `any` and `all` together
  const uint32_t* outc;   // [string row][n] outcome ids
  const uint32_t* truth;  // [condition][words] bit planes over outcome ids
  const uint32_t* unk;
  const uint32_t* err;    // [string row][words]: the outcome is a substitution error / outside the device
  const uint32_t* oos;    // scope (read by the strict fold only: may be null for a gate)
  uint32_t words;
};

// result of the fold: the block's value, and (strict) whether a string of it is an error / outside the scope
constexpr uint32_t KV_FOLD_FALSE = 0u, KV_FOLD_TRUE = 1u, KV_FOLD_UNKNOWN = 2u, KV_FOLD_VALUE = 3u;
constexpr uint32_t KV_FOLD_ERR = 4u, KV_FOLD_OOS = 8u;

// Block `set` on item i of n (a resource of the batch, an element of a foreach list): the any / all
// fold with three-valued logic (evaluate.go:42-78: `any` absent is true, `all` absent or empty is
// true, the result their AND; the reference's short-circuit has no side effects, so a result the
// known conditions decide is exact). A lane loads the outcome id of each string of the block once
// (outc[string][i], coalesced; the entries are ordered by string) and tests it in the truth and
// unknown planes of the string's conditions. STRICT (the strict resolver: deny blocks): the outcome
// is also tested in the string's error and out-of-scope planes, whatever the fold's short-circuit
// would have skipped (substitution covers the whole block first, vars.go:315-317), so a constant
// false block still walks its strings. The set's entry list is the same for every lane of a wave
// (scalar loads on the device).
template <bool STRICT>
KV_HD inline uint32_t kv_cond_fold(const CondBlocks& T, uint32_t set, uint64_t n, uint64_t i) {
  const uint32_t first = T.sets[4 * set], cnt = T.sets[4 * set + 1], flags = T.sets[4 * set + 2];
  if (!STRICT && (flags & KV_SET_FALSE)) return KV_FOLD_FALSE;
  bool any_t = false, any_u = false, all_f = false, all_u = false, e = false, x = false;
  uint32_t cur = 0xFFFFFFFFu, o = 0;
  for (uint32_t k = 0; k < cnt; k++) {
    const uint32_t cs = T.ents[2 * (first + k)], cw = T.ents[2 * (first + k) + 1];
    if (cs != cur) {
      cur = cs;
      o = T.outc[(uint64_t)cs * n + i];
      if (STRICT) {
        const uint64_t sw = (uint64_t)cs * T.words + (o >> 5);
        e |= (T.err[sw] >> (o & 31u)) & 1u;
        x |= (T.oos[sw] >> (o & 31u)) & 1u;
      }
    }
    const uint32_t c = cw & ~KV_ENT_ALL;
    // (bare entries exist only under the strict resolver; without the test the gate's loop has no
    // path that leaves a loaded outcome id unused, which would cost the callers a wait on their
    // own loads in flight)
    if (STRICT && c == KV_ENT_NOCOND) continue;
    const uint64_t w = (uint64_t)c * T.words + (o >> 5);
    const bool t = (T.truth[w] >> (o & 31u)) & 1u, u = (T.unk[w] >> (o & 31u)) & 1u;
    if (cw & KV_ENT_ALL) {
      all_f |= !t && !u;
      all_u |= u;
    } else {
      any_t |= t;
      any_u |= u;
    }
  }
  const bool any_present = (flags & KV_SET_ANY) != 0u;
  const bool any_false = any_present && !any_t && !any_u;
  const bool any_unknown = any_present && !any_t && any_u;
  const uint32_t v = (flags & KV_SET_FALSE) || any_false || all_f ? KV_FOLD_FALSE
                     : any_unknown || all_u                      ? KV_FOLD_UNKNOWN
                                                                 : KV_FOLD_TRUE;
  return v | (e ? KV_FOLD_ERR : 0u) | (x ? KV_FOLD_OOS : 0u);
}

// The gate's verdict: 0 (the preconditions hold), ST_SKIP (they do not) or ST_CPU (undecided: a
// map / array operand on this item).
KV_HD inline uint32_t kv_gate_status(uint32_t fold) {
  return fold == KV_FOLD_FALSE ? ST_SKIP : fold == KV_FOLD_UNKNOWN ? ST_CPU : 0u;
}

// The deny verdict, in this order:
//   a string outside the device scope on this item              -> ST_CPU
//   a string whose variables do not resolve (vars.go:315-317)   -> ST_ERROR
//   the conditions hold -> ST_FAIL, do not hold -> ST_PASS (validation.go:315-320)
//   undecided (a map / array operand)                           -> ST_CPU
KV_HD inline uint32_t kv_deny_status(uint32_t fold) {
  if (fold & KV_FOLD_OOS) return ST_CPU;
  if (fold & KV_FOLD_ERR) return ST_ERROR;
  const uint32_t v = fold & KV_FOLD_VALUE;
  return v == KV_FOLD_FALSE ? ST_PASS : v == KV_FOLD_UNKNOWN ? ST_CPU : ST_FAIL;
}

}  // namespace kv
