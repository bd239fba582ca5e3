// The precondition gate of one (condition set, resource): shared by kv_precond_kernel
// (kvkernel.hip), the host (kvcond.cpp pre_status_host) and the host harness tools/kvemu.
// Plain code over the tables of kvcond.h PreHost / DevBatch::pre_*; needs kv_layout.h.
#pragma once

namespace kv {

// Folds the set's conditions with three-valued logic (evaluate.go:42-78: `any` absent is true,
// `all` absent or empty is true, the result their AND; the reference's short-circuit has no side
// effects, so a result the known conditions decide is exact). Per condition: the lane's outcome
// id of the condition's string (outc[string][res], reloaded only when the string changes: the
// entries are ordered by string), then its truth and unknown bits. Returns 0 (the preconditions
// hold), ST_SKIP (they do not) or ST_CPU (undecided: a map / array operand on this resource).
// The set's entry list is the same for every lane of a wave (scalar loads on the device).
KV_HD inline uint32_t kv_pre_lane(const uint32_t* __restrict__ sets, const uint32_t* __restrict__ ents,
                                  const uint32_t* __restrict__ outc, const uint32_t* __restrict__ truth,
                                  const uint32_t* __restrict__ unk, uint32_t words, uint32_t set, uint64_t n_res,
                                  uint64_t r) {
  const uint32_t first = sets[4 * set], wa = sets[4 * set + 1], n_all = sets[4 * set + 2];
  if (sets[4 * set + 3]) return ST_SKIP;  // a constant condition decides
  const uint32_t n_any = wa & 0x7FFFFFFFu;
  const bool any_present = (wa >> 31) != 0u;
  bool any_t = false, any_u = false, all_f = false, all_u = false;
  uint32_t cur = 0xFFFFFFFFu, o = 0;
  for (uint32_t i = 0; i < n_any + n_all; i++) {
    const uint32_t cs = ents[2 * (first + i)], c = ents[2 * (first + i) + 1];
    if (cs != cur) {
      cur = cs;
      o = outc[(uint64_t)cs * n_res + r];
    }
    const uint64_t w = (uint64_t)c * words + (o >> 5);
    const bool t = (truth[w] >> (o & 31u)) & 1u, u = (unk[w] >> (o & 31u)) & 1u;
    if (i < n_any) {
      any_t |= t;
      any_u |= u;
    } else {
      all_f |= !t && !u;
      all_u |= u;
    }
  }
  const bool any_false = any_present && !any_t && !any_u;
  const bool any_unknown = any_present && !any_t && any_u;
  if (any_false || all_f) return ST_SKIP;
  if (any_unknown || all_u) return ST_CPU;
  return 0u;
}

}  // namespace kv
