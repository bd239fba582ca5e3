// Rule preconditions (pkg/engine/validation.go:175-193 checkPreconditions -> utils.go:445-458):
// the condition evaluator of pkg/engine/variables/operator/*.go on the host, the compiled form
// of a policy set's precondition blocks, and the per-batch tables the device gate reads.
//
// The reference substitutes the preconditions document per (rule, resource)
// (SubstituteAllInPreconditions, vars.go:62-84: an unresolved variable becomes ""), converts it
// to kyverno.Condition values (pkg/utils/util.go:220-262: numbers are float64) and evaluates
// any / all (variables/evaluate.go:42-78). Here:
//  * compile (kvcond.cpp compile_preconditions): conditions and condition sets are interned
//    across all rules; a condition is (variable string | constant, operator, constant); the
//    ones without variables are folded. RuleRec::pre = 1 + set index;
//  * ingest: every distinct condition string resolves once per resource into the batch's outcome
//    table (Batch::vout columns after the pattern variables', kvvars.cpp resolver mode);
//  * per batch (build_pre): every condition is evaluated once per *distinct* outcome its string
//    takes, into two bit planes indexed by outcome id (truth, unknown);
//  * device (kvpre.h kv_pre_lane, kv_precond_kernel): one lane per resource folds its set's
//    conditions with three-valued logic into DevBatch::pre_st[set][res].
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "kvinternal.hpp"

namespace kvh {

// operators (operator.go:28-78, names compare case-insensitively); CD_UNKNOWN: constant false
// (evaluate.go:13-16), CD_DURATION: the deprecated Duration* handlers (outside the scope)
enum CondOp : uint32_t {
  CD_UNKNOWN = 0, CD_EQ, CD_NE, CD_IN, CD_NOTIN, CD_ANYIN, CD_ALLIN, CD_ANYNOTIN, CD_ALLNOTIN,
  CD_GT, CD_GE, CD_LT, CD_LE, CD_DURATION
};
uint32_t cond_op(const std::string& name);

// time.ParseDuration (nanoseconds)
bool go_parse_duration(const std::string& s, int64_t* out);

// variables.Evaluate on substituted operands (numbers float64, nil = J_NULL). Returns false with
// *range = true for operands outside the scope (a map, a list key, a list holding maps / lists,
// Duration* operators).
bool cond_eval(uint32_t op, const PV& key, const PV& value, bool* range);

// Parses the `preconditions` node of a rule. Returns 0 when the block is outside the device scope
// (the rule stays CPU-routed, reason "preconditions"), else 1 + the interned set's index, or
// 0xFFFFFFFF when the block always passes (no gate).
uint32_t compile_preconditions(PolicySet& ps, const JDoc& d, uint32_t node);

// Per-batch tables of the gate (device layout, DevBatch::pre_*).
struct PreHost {
  std::vector<uint32_t> sets;   // 4 words per set: first entry, n_any | any_present << 31, n_all, const_false
  std::vector<uint32_t> ents;   // 2 words per entry: condition string, condition (plane row); any then all
  std::vector<uint32_t> outc;   // outcome id per [condition string][res]
  std::vector<uint32_t> truth, unk;  // [condition][words] bit planes over outcome ids
  uint32_t words = 1;
};
void build_pre(const PolicySet& ps, const Batch& b, PreHost* out);
// the gate of one (set, resource) on the host: 0 pass, ST_SKIP, ST_CPU (as kv_pre_lane)
uint8_t pre_status_host(const PreHost& h, uint32_t set, uint64_t n_res, uint64_t r);

}  // namespace kvh
