// validate.deny of one (deny set, resource): shared by kv_deny_kernel (kvkernel.hip), the host
// (kvcond.cpp deny_status_host) and the host harness tools/kvemu. Plain code over the tables of
// kvcond.h DenyHost / DevBatch::deny_*; needs kv_layout.h.
#pragma once

namespace kv {

constexpr uint32_t KV_DENY_ALL = 0x80000000u;     // entry word 1: the condition is a member of `all`
constexpr uint32_t KV_DENY_NOCOND = 0x7FFFFFFFu;  // entry word 1: the string has no condition to evaluate

// The set's entries are ordered by condition string, so a lane loads the outcome id of each
// string once (outc[string][res], coalesced) and tests it in that string's error and
// out-of-scope planes; the entry's condition, if any, adds its truth / unknown bits to the
// three-valued any / all fold of kv_pre_lane (evaluate.go:42-78). Verdict, in this order:
//   a string outside the device scope on this resource            -> ST_CPU
//   a string whose variables do not resolve (vars.go:315-317)     -> ST_ERROR (whatever the
//     fold's short-circuit would have skipped: substitution covers the whole block first)
//   the conditions hold -> ST_FAIL, do not hold -> ST_PASS (validation.go:315-320)
//   undecided (a map / array operand)                             -> ST_CPU
// The set's entry list is the same for every lane of a wave (scalar loads on the device).
KV_HD inline uint32_t kv_deny_lane(const uint32_t* __restrict__ sets, const uint32_t* __restrict__ ents,
                                   const uint32_t* __restrict__ outc, const uint32_t* __restrict__ truth,
                                   const uint32_t* __restrict__ unk, const uint32_t* __restrict__ err,
                                   const uint32_t* __restrict__ oos, uint32_t words, uint32_t set, uint64_t n_res,
                                   uint64_t r) {
  const uint32_t first = sets[4 * set], n = sets[4 * set + 1];
  const bool any_present = sets[4 * set + 2] != 0u, const_false = sets[4 * set + 3] != 0u;
  bool any_t = false, any_u = false, all_f = false, all_u = false, e = false, x = false;
  uint32_t cur = 0xFFFFFFFFu, o = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t cs = ents[2 * (first + i)], cw = ents[2 * (first + i) + 1];
    if (cs != cur) {
      cur = cs;
      o = outc[(uint64_t)cs * n_res + r];
      const uint64_t sw = (uint64_t)cs * words + (o >> 5);
      e |= (err[sw] >> (o & 31u)) & 1u;
      x |= (oos[sw] >> (o & 31u)) & 1u;
    }
    const uint32_t c = cw & ~KV_DENY_ALL;
    if (c == KV_DENY_NOCOND) continue;
    const uint64_t w = (uint64_t)c * words + (o >> 5);
    const bool t = (truth[w] >> (o & 31u)) & 1u, u = (unk[w] >> (o & 31u)) & 1u;
    if (cw & KV_DENY_ALL) {
      all_f |= !t && !u;
      all_u |= u;
    } else {
      any_t |= t;
      any_u |= u;
    }
  }
  if (x) return ST_CPU;
  if (e) return ST_ERROR;
  if (const_false) return ST_PASS;
  const bool any_false = any_present && !any_t && !any_u;
  const bool any_unknown = any_present && !any_t && any_u;
  if (any_false || all_f) return ST_PASS;
  if (any_unknown || all_u) return ST_CPU;
  return ST_FAIL;
}

}  // namespace kv
