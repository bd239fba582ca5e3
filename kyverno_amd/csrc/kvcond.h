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
//  * device (kvblocks.h kv_cond_fold, kv_precond_kernel): one lane per resource folds its set's
//    conditions with three-valued logic into DevBatch::pre_st[set][res].
// validate.deny and the two blocks of a validate.foreach entry (below) are the same machinery with
// another resolver and another verdict: one table form (CondHost, kvblocks.h CondBlocks), one
// entry packer, one plane filler and one fold serve all three.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "kvinternal.hpp"

namespace kv {
struct CondBlocks;  // kvblocks.h
struct FeTables;    // kvforeach.h
struct FePatTables;
struct FeAnyTables;
struct FeVarTables;
}

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

// Per-batch tables of the condition blocks of one space (the device layout: kvblocks.h CondBlocks).
struct CondHost {
  std::vector<uint32_t> sets;   // 4 words per set: first entry, entries, KV_SET_* flags, 0
  std::vector<uint32_t> ents;   // 2 words per entry: string row, condition | KV_ENT_ALL, or KV_ENT_NOCOND; by string
  std::vector<uint32_t> outc;   // outcome id per [string row][item]
  std::vector<uint32_t> truth, unk;  // [condition][words] bit planes over outcome ids
  std::vector<uint32_t> err, oos;    // [string row][words]: the outcome is an error / outside the device scope
                                     // (rows of strings under the preconditions resolver stay empty; no such
                                     // planes at all for the gate)
  uint32_t words = 1;
  kv::CondBlocks view() const;
};
void build_pre(const PolicySet& ps, const Batch& b, CondHost* out);
// the gate of one (set, resource) on the host: 0 pass, ST_SKIP, ST_CPU (as kv_precond_kernel)
uint8_t pre_status_host(const CondHost& h, uint32_t set, uint64_t n_res, uint64_t r);

// validate.deny on the device (KV_COMPILE_DENY; pkg/engine/validation.go:299-339 validateDeny).
// The reference substitutes the deny conditions per (rule, resource) with the default resolver
// (variables.SubstituteAll, vars.go:76-80,315-317: an unresolved variable is an error, and the
// whole document is substituted before anything is evaluated), converts them as the preconditions
// (utils.go:392-406) and evaluates the same any / all fold: true is FAIL, false is PASS. Here the
// preconditions' machinery runs with another resolver and another verdict, and no pattern walk:
//  * compile (compile_deny): blocks, conditions and strings are interned in tables of their own
//    (PolicySet::dsets / deny). A block whose conditions fold to a constant is still a
//    deny set, so preconditions compose with it. The strings are keyed by their text alone: the
//    string's path inside the conditions document shows only in the reference's non-NotFound
//    errors, all of which are outside the device scope here (outcome "C");
//  * ingest: deny strings resolve with the strict resolver into further columns of Batch::vout;
//  * per batch (build_deny): truth / unknown planes per condition as for the preconditions, and
//    per string an error plane (the outcome is a substitution error) and an out-of-scope plane;
//  * device (kvblocks.h kv_cond_fold<strict> + kv_deny_status, kv_deny_kernel):
//    DevBatch::deny_st[set][res], the final status of the pair once match / exclude and the
//    preconditions let it through.
// Parses the `deny` node of a rule: 0 when it is outside the device scope (the rule stays
// CPU-routed, reason "deny"), else 1 + the interned deny set's index.
uint32_t compile_deny(PolicySet& ps, const JDoc& d, uint32_t node);

void build_deny(const PolicySet& ps, const Batch& b, CondHost* out);
// one (deny set, resource) on the host: ST_PASS, ST_FAIL, ST_ERROR or ST_CPU (as kv_deny_kernel)
uint8_t deny_status_host(const CondHost& h, uint32_t set, uint64_t n_res, uint64_t r);
// the error of the first unresolved string of the set on store resource r, in the order of the
// reference's traversal with canonical key order ("" when every string resolves)
std::string deny_error_host(const PolicySet& ps, const Batch& b, uint32_t set, uint64_t r);

// validate.foreach on the device (KV_COMPILE_FOREACH; pkg/engine/validation.go:108-115,204-283
// validateForEach). The reference queries the entry's `list` on the JSON context, and per element,
// in order, merges {"element": <element>} into the context and runs validate() with the entry's
// preconditions (preconditions resolver) and deny block (strict resolver): a SKIP is ignored, the
// first result that is neither PASS nor SKIP ends the rule; without one the rule is PASS when an
// element passed, else SKIP "rule skipped". Scope: one entry {list, preconditions?, deny} per
// rule (with several entries, keys of the previous entry's last element leak into `element`
// through the merge patch: KV_COMPILE_FOREACH_ENTRIES, compile_foreach below, restates that),
// preconditions a map (the old list form is dropped by the reference),
// variables `{{element<chain>}}` / `{{request.object<chain>}}`. DESIGN.md §3 *Foreach*.
//  * compile (compile_foreach): lists, element-scoped strings (per list and resolver mode; a
//    string with request.object variables only is an element-scoped string too: one key space,
//    one resolver call site), conditions and foreach sets are interned in PolicySet::f* / elem;
//  * ingest: per (resource, list) the list state and element count, per (element, string) an
//    outcome id of the batch's outcome table, element-major (Batch::fstate / fcount / fout);
//  * per batch (build_foreach): the entries and planes of build_deny / build_pre over the element
//    strings (a string row per (list, string)), the outcome ids transposed to [string][element],
//    el_res / el_ord per element;
//  * device (kvforeach.h, kv_foreach_elem_kernel, kv_foreach_fin_kernel): a lane per element, a
//    segmented first-decisive-element reduction into 32-bit keys, a byte per (set, resource) in
//    the rows of DevBatch::deny_st after the deny sets'.
// Pattern entries (KV_COMPILE_FOREACH_PATTERN; validation.go:187-193,341-345,421-445: with
// `pattern` set the element's validate() ends in MatchPattern(element, pattern), the element map as
// the whole resource). Scope: one entry {list, preconditions?, pattern}, the pattern a map without
// {{ }} variables and without a `metadata` key, inside what the pattern compiler accepts.
//  * compile: the pattern is compiled by the pattern compiler (kvcompile.cpp) rooted at the
//    projection-trie node of the list's elements, so the projection keeps the pattern's keys under
//    them; a foreach set is then (list, gate, pattern program + root pattern node), interned like
//    the others; PolicySet::fchains holds the list's path as the device walks it;
//  * device (kvwalk.h, kv_foreach_pat_kernel): a lane per element finds its element's node along
//    the list path, runs the entry gate and the bytecode walk of kv_validate_kernel with the element
//    as the root, and feeds its code into the reduction of kv_foreach_elem_kernel; the deciding
//    element's 8-byte error record goes to fe_rec[pattern set][res] (kv_foreach_rec_kernel).
//  * An element whose verdict the int64 / float64 typing of a number could change (the element
//    comes out of the JSON context: every number float64) is ST_CPU: kvwalk.h.
// Parses the `validate.foreach` node of a rule: 0 when it is outside the device scope (the rule
// stays CPU-routed, reason "foreach"), else 1 + the interned foreach set's index. `pattern`
// (KV_COMPILE_FOREACH_PATTERN; null: pattern entries stay outside the scope) compiles the entry's
// pattern node for list `list` (index `list_index`) into s->prog / s->root_pnode and records the
// list's path (PolicySet::fchains); false: outside the scope (no instruction or set is left behind; kvcompile.cpp).
using FePatternCompiler = std::function<bool(uint32_t pattern_node, const std::string& list, uint32_t list_index, FeSet* s)>;
// `chain` (KV_COMPILE_FOREACH_ENTRIES; null: a rule of several entries stays outside the scope): a
// list of 2 to 16 entries, each what a single entry may be, compiles to a *chain*, the ordered
// list of its entries' foreach sets (PolicySet::fe_chains); the return value is then 0 and
// *chain = 1 + the interned chain. The reference's context keeps the last element of entry k
// merged in when entry k + 1 starts (DESIGN.md §3 *Several entries*), so the element strings of an
// entry behind the first are interned per *leak context*, the lists of the entries before it
// (PolicySet::fctx), and resolve at ingest against the element over those lists' last elements.
// `anypattern` (KV_COMPILE_FOREACH_ANYPATTERN, with `pattern`; validation.go:175-202,447-489): an
// entry {list, preconditions?, anyPattern} of 1 to 8 map alternatives compiles to an *any set*, a
// foreach set with one plain pattern program per alternative (each compiled by `pattern`, with a
// root pattern node of its own), interned by the alternatives' texts. Per element the device
// tries them in order (kv_foreach_any_kernel): the first that matches is PASS, none is FAIL.
// `patvars` (KV_COMPILE_FOREACH_PATVARS, with `pattern`): a pattern or an alternative may hold
// `{{element...}}` / `{{request.object...}}` variables in its string values. Each such string is a
// strict element string of the entry's list in its leak context (FeSet::vorder: the substitution's
// traversal order), a leaf on it a dynamic leaf that names the string's row (OP_VLEAF). Per element
// the device takes the substitution verdict first (kvforeach.h kv_fe_subst: an unresolved variable
// is ST_ERROR "variable substitution failed", validation.go:549-571), then walks the pattern with
// the element's substituted values (kvwalk.h). `pattern` reads s->list and s->ctx.
uint32_t compile_foreach(PolicySet& ps, const JDoc& d, uint32_t node, const FePatternCompiler* pattern = nullptr,
                         uint32_t* chain = nullptr, bool anypattern = false, bool patvars = false);

struct FeHost {
  // row s of gate / deny: the entry preconditions / the deny block of foreach set s. deny holds the
  // outcome ids and every plane; gate only sets and entries (its view reads deny's outc, truth, unk)
  CondHost gate, deny;
  std::vector<uint32_t> sets, lists, el_res, el_ord, lstate;  // kvforeach.h FeTables
  std::vector<uint32_t> first;  // [list][res]: the resource's first element in the list's block (the host
                                // accessors; on the device only kv_foreach_rec_kernel reads it)
  std::vector<uint32_t> pats, chain;  // kvforeach.h FePatTables: the pattern sets and their lists' paths
  std::vector<uint32_t> chains, chain_ents;  // kvforeach.h FeTables: the rules of several entries
  std::vector<uint32_t> anys, any_alts;      // kvforeach.h FeAnyTables: the any sets and their alternatives' programs
  // kvforeach.h FeVarTables (KV_COMPILE_FOREACH_PATVARS; all empty without a set that has variable
  // strings): a run per pattern set, then per any set; the runs' string rows; the M plane
  std::vector<uint32_t> vruns, vrows, mpl;
  bool has_vars() const { return !vrows.empty(); }
  // (ityp: the int-typing plane of the batch predicate table, DynHost::ityp)
  kv::FeVarTables var_view(const uint32_t* ityp) const;
  uint32_t max_el = 0;
  kv::FeTables view() const;
  kv::FePatTables pat_view() const;
  kv::FeAnyTables any_view() const;
};
void build_foreach(const PolicySet& ps, const Batch& b, FeHost* out);
// one (foreach set, store resource) on the host, as the two kernels: ST_PASS, ST_FAIL, ST_ERROR,
// ST_SKIP or ST_CPU; *elem the deciding element's index in its list, 0xFFFFFFFF without one.
// Throws for a pattern set (its elements are walked on the device only)
uint8_t foreach_fold_host(const FeHost& h, uint32_t set, uint64_t n_res, uint64_t r, uint32_t* elem);
// one (chain, store resource) on the host, as kv_foreach_chain_kernel over the rows
// foreach_fold_host gives: the status, *entry the deciding entry (0xFFFFFFFF without one) and *elem
// its deciding element. Throws where an entry is a pattern set
// (`scratch`: kept by a caller that folds many resources, so nothing is allocated per resource)
struct FeChainScratch {
  std::vector<uint32_t> acc, ls;
};
uint8_t foreach_chain_fold_host(const FeHost& h, uint32_t chain, uint64_t n_res, uint64_t r, uint32_t* entry, uint32_t* elem,
                                FeChainScratch* scratch = nullptr);
// the error of the first unresolved deny string of element `elem` of store resource r, in the
// order of deny_error_host
std::string foreach_error_host(const PolicySet& ps, const Batch& b, const FeHost& h, uint32_t set, uint64_t r,
                               uint32_t elem);
// KV_COMPILE_FOREACH_PATVARS: the substitution verdict of element `elem` of store resource r under
// the pattern strings of `set` (a pattern set or an any set), as the kernels take it
// (kv_fe_subst): 0, ST_ERROR or ST_CPU ...
uint32_t foreach_subst_host(const FeHost& h, uint32_t set, uint64_t n_res, uint64_t r, uint32_t elem);
// ... and the error of the first unresolved pattern string in traversal order ("" without one)
std::string foreach_subst_error_host(const PolicySet& ps, const Batch& b, const FeHost& h, uint32_t set, uint64_t r,
                                     uint32_t elem);
// the outcome (Batch::vout_tab index) of element string `key` (PolicySet::fkeys) on that element
uint32_t foreach_elem_outcome(const PolicySet& ps, const Batch& b, const FeHost& h, uint32_t key, uint64_t r, uint32_t elem);

}  // namespace kvh
