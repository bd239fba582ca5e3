/*
 * kvgpu.h — C ABI of the MI355X-native batch validate.pattern engine.
 *
 * Drop-in boundary for Kyverno's validate hot path (isabella232/kyverno v1.5.x):
 *   engine.Validate(policyContext *PolicyContext) *response.EngineResponse
 *       pkg/engine/validation.go:26
 * called per (policy, resource) by
 *   CLI apply        pkg/kyverno/common/common.go:541 (loop at pkg/kyverno/apply/apply_command.go:270-310)
 *   background scan  pkg/policy/apply.go:72 (via pkg/policy/existing.go:55-58)
 *   test runner      pkg/testrunner/scenario.go:169
 * The batch form evaluates every (resource, rule) pair of a policy set at once.
 * Plain C types only; all handles are opaque and library-owned until kv_free_*.
 * Return value: 0 on success, negative KV_E_* on failure (with *err set when
 * err != NULL; free with kv_free_error). Per-pair evaluation never fails: it
 * yields status KV_STATUS_ERROR exactly like the reference.
 */
#ifndef KVGPU_H
#define KVGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* response.RuleStatus (pkg/engine/response/status.go:14-28) + batch extras */
enum {
  KV_STATUS_PASS = 0,
  KV_STATUS_FAIL = 1,
  KV_STATUS_WARN = 2,
  KV_STATUS_ERROR = 3,
  KV_STATUS_SKIP = 4,
  KV_STATUS_NOMATCH = 5, /* no RuleResponse: rule not matched / not a pattern rule (CLI counts skip) */
  KV_STATUS_CPU = 6      /* route the pair to the reference CPU engine (processValidationRule) */
};

/* rule routes decided at compile time */
enum { KV_ROUTE_GPU = 0, KV_ROUTE_CPU = 1, KV_ROUTE_NORESPONSE = 2, KV_ROUTE_CONSTANT = 3 };

/* kv_compile flags */
enum {
  /* also lower every rule to a specialized gfx950 kernel (hiprtc, at compile
   * time); kv_validate/kv_session then run those instead of the bytecode VM */
  KV_COMPILE_SPECIALIZE = 1,
  /* evaluate validate.deny rules on the device (opt-in; without it every such rule is
   * KV_ROUTE_CPU, reason "deny"). In scope: a rule with validate.deny and no pattern /
   * anyPattern, context or foreach, preconditions absent or of the device forms, and
   * deny.conditions an any / all block (or the old list) whose conditions are of the forms the
   * preconditions accept: a request.object variable string on one side, a constant scalar or
   * list on the other, or both constant. A pair is FAIL when the conditions hold, PASS when they
   * do not, ERROR when a variable of the block does not resolve (kv_result_deny_message), CPU
   * when the device cannot decide (a map or array operand). Other forms keep the CPU route. */
  KV_COMPILE_DENY = 2,
  /* evaluate validate.foreach rules on the device (opt-in, independent of KV_COMPILE_DENY;
   * without it every such rule is KV_ROUTE_CPU, reason "foreach"). In scope: validate.foreach a
   * list of exactly one entry {list, preconditions?, deny} with nothing beside it in validate and
   * no rule-level context; rule preconditions absent or of the device forms; `list` a bare
   * request.object field / quoted-field / index chain; deny.conditions as KV_COMPILE_DENY
   * accepts them and the entry's preconditions a map of any / all of the device forms, both over
   * {{element<chain>}} and {{request.object<chain>}} variables. Per pair: the elements are
   * evaluated in order; the first FAIL (the conditions hold), ERROR (a deny variable does not
   * resolve) or CPU (the device cannot decide) element is the pair's status; else PASS when an
   * element passed, SKIP "rule skipped" when the list is missing or empty or every element is
   * gated by the entry's preconditions. CPU also when the list is not a list of maps (or a
   * map), holds a null anywhere, or has more than 65536 elements. */
  KV_COMPILE_FOREACH = 4,
  /* also evaluate validate.foreach entries that carry a `pattern` on the device (opt-in; needs
   * KV_COMPILE_FOREACH, else kv_compile returns KV_E_INVALID; without it such a rule is
   * KV_ROUTE_CPU, reason "foreach"). In scope: one entry {list, preconditions?, pattern}, the
   * pattern a map without {{ }} variables (KV_COMPILE_FOREACH_PATVARS lifts that) and without a
   * `metadata` key, inside what the pattern
   * compiler accepts for a rule's pattern. Per element the pattern is matched with the element as
   * the whole resource (validate.MatchPattern): no error is PASS, a conditional / global anchor
   * skip is SKIP (ignored by foreach), an error without a path ERROR, any other FAIL with a path
   * relative to the element (kv_result_foreach_path); the first FAIL / ERROR / CPU element
   * decides as for deny entries. The reference compares every number of an element as float64;
   * an element holding an int64-typed number where that typing could change the verdict (a
   * string pattern compared on the number's text form, |n| >= 2^53) is CPU, as is an error
   * record that does not fit 8 bytes. */
  KV_COMPILE_FOREACH_PATTERN = 8,
  /* also evaluate validate.foreach rules of 2 to 16 entries on the device (opt-in; needs
   * KV_COMPILE_FOREACH, else kv_compile returns KV_E_INVALID; composes with
   * KV_COMPILE_FOREACH_PATTERN; without it such a rule is KV_ROUTE_CPU, reason "foreach"). Every
   * entry must be what a single entry may be under the other two flags; deny and pattern entries
   * may mix. The entries run in order with one applyCount: the first FAIL / ERROR / CPU element
   * of the first entry that has one decides (kv_result_foreach_entry, kv_result_foreach_element),
   * else PASS when an element of any entry passed, else SKIP "rule skipped"; an entry whose list
   * is outside the device scope makes the pair CPU unless an earlier entry decided. As in the
   * reference, the last element of entry k stays merged into the context when entry k + 1 starts:
   * the {{element...}} variables of a later entry's preconditions, deny conditions and message read
   * the element merged over the last elements of the lists before it (maps merge key by key,
   * anything else replaces); an entry's pattern sees the raw element. */
  KV_COMPILE_FOREACH_ENTRIES = 16,
  /* also evaluate validate.foreach entries that carry an `anyPattern` on the device (opt-in; needs
   * KV_COMPILE_FOREACH | KV_COMPILE_FOREACH_PATTERN, else kv_compile returns KV_E_INVALID;
   * composes with KV_COMPILE_FOREACH_ENTRIES; without it such a rule is KV_ROUTE_CPU, reason
   * "foreach"). In scope: an entry {list, preconditions?, anyPattern}, anyPattern a list of 1 to 8
   * maps, each within the limits of a pattern entry, no $() reference anywhere in the list (the
   * reference resolves those against the list as a whole). Per element the alternatives are tried in
   * order as MatchPattern(element, alternative): the first that matches makes the element PASS,
   * none makes it FAIL (never SKIP or ERROR); the rule verdict is the foreach reduction. For the
   * deciding element of a FAIL pair every alternative's outcome is kept
   * (kv_result_foreach_alt). An element is CPU where an alternative up to and including the
   * first that passes meets the typing guard of pattern entries or a record that does not fit
   * 8 bytes. */
  KV_COMPILE_FOREACH_ANYPATTERN = 32,
  /* also evaluate validate.foreach entries whose `pattern` (or, with KV_COMPILE_FOREACH_ANYPATTERN,
   * `anyPattern`) holds {{ }} variables on the device (opt-in; needs KV_COMPILE_FOREACH |
   * KV_COMPILE_FOREACH_PATTERN, else kv_compile returns KV_E_INVALID; composes with the anyPattern
   * and entries flags; without it such a rule is KV_ROUTE_CPU, reason "foreach"). In scope: string
   * values holding {{element<field / quoted-field / index chain>}} and {{request.object<chain>}},
   * as the whole string (the value keeps its JSON type, numbers float64) or inside one (spliced
   * text), several per string. Outside it: a variable in a map key, {{element}} alone, {{@}},
   * functions, nested variables, \{{ escapes, a $() reference that brings a variable in. Per
   * element, after the entry's preconditions, the whole pattern (every alternative of an
   * anyPattern, alternative 0's strings first) is substituted in the element's context (in a rule
   * of several entries: the element over the last elements of the lists before it): the first
   * string in traversal order that does not resolve makes the element ERROR "variable substitution
   * failed: <err>" (kv_result_foreach_subst_error), one outside the resolver's scope CPU, else a
   * map or an array in a leaf's place CPU; then the substituted pattern is matched against the
   * element. The typing guard of pattern entries is decided per substituted value. */
  KV_COMPILE_FOREACH_PATVARS = 64
};

/* kv_validate modes (bit set). KV_MODE_SCOPES adds per-scope counts
 * (scope = namespace; "" = cluster scope), the PolicyReport / ClusterPolicyReport
 * summaries of pkg/kyverno/apply/report.go:76-179 and the background controller's
 * pkg/policyreport/builder.go:245-308; the specialized kernels count them inside the
 * pass (no status matrix unless KV_MODE_STATUS / KV_MODE_ERRORS is asked for too). */
enum { KV_MODE_STATUS = 1, KV_MODE_ERRORS = 2, KV_MODE_COUNTS = 4, KV_MODE_SCOPES = 8 };

enum { KV_E_INVALID = -1, KV_E_PARSE = -2, KV_E_DEVICE = -3, KV_E_RANGE = -4, KV_E_NOMEM = -5 };

typedef struct kv_policyset kv_policyset;
typedef struct kv_batch kv_batch;
typedef struct kv_result kv_result;
typedef struct kv_error {
  int code;
  char* message;
} kv_error;

typedef struct kv_rule_info {
  uint32_t policy;          /* index of the policy in the compiled list */
  const char* policy_name;  /* metadata.name */
  const char* name;         /* rule name */
  uint32_t route;           /* KV_ROUTE_* */
  const char* route_reason; /* why CPU / no-response ("" for GPU) */
  const char* message;      /* validate.message */
  uint32_t any_pattern;     /* 1 for anyPattern rules */
  uint32_t const_status;    /* KV_ROUTE_CONSTANT */
  const char* const_message;
  uint32_t foreach_set;     /* 1 + the foreach set of a device foreach rule (KV_COMPILE_FOREACH), else 0 */
} kv_rule_info;

/* Compile a JSON list of ClusterPolicy/Policy objects (already through
 * policymutation autogen, as the reference CLI does before engine.Validate).
 * Replaces the per-call interpretation in pkg/engine/validate, pkg/engine/anchor,
 * pkg/engine/operator and the $() reference substitution of
 * pkg/engine/variables/vars.go:253-309. */
int kv_compile(const char* policies_json, size_t len, uint32_t flags, kv_policyset** out, kv_error** err);
int kv_policyset_info(const kv_policyset* ps, uint32_t* n_policies, uint32_t* n_rules);
/* specialized kernels of a KV_COMPILE_SPECIALIZE policy set (zeros otherwise) */
int kv_policyset_jit_info(const kv_policyset* ps, uint32_t* n_kernels, double* gen_ms, double* compile_ms,
                          uint64_t* code_bytes);
/* path columns the specialized kernels read, by cell format: wide (12 or 16 bytes a cell) and
 * narrow (4 bytes: presence, type and a scalar's value id) */
int kv_policyset_jit_cols(const kv_policyset* ps, uint32_t* n_wide, uint32_t* n_narrow);
/* rule preconditions evaluated on the device: interned condition sets, conditions with a
 * variable operand, and distinct condition strings of the policy set (any may be NULL) */
int kv_policyset_cond_sets(const kv_policyset* ps, uint32_t* sets, uint32_t* conditions, uint32_t* strings);
/* Evaluates one already-substituted condition {"key":..., "operator":..., "value":...} as
 * variables.Evaluate does (pkg/engine/variables/evaluate.go:11-18, operator/*.go), numbers as
 * float64: *result = 0 or 1. KV_E_RANGE when an operand is outside the device scope (a map, a
 * list key, the deprecated Duration* operators), KV_E_PARSE for bad JSON. Needs no GPU. */
int kv_condition_eval(const char* condition_json, size_t len, int* result);
/* validate.deny rules evaluated on the device (KV_COMPILE_DENY): interned deny sets, their
 * conditions with a variable operand, and their distinct condition strings (a key space apart
 * from the preconditions': deny strings resolve under the strict resolver). Any may be NULL. */
int kv_policyset_deny_sets(const kv_policyset* ps, uint32_t* sets, uint32_t* conditions, uint32_t* strings);
/* *set = 1 + the deny set of rule `rule`, 0 for a rule that is not a device deny rule */
int kv_rule_deny_set(const kv_policyset* ps, uint32_t rule, uint32_t* set);
/* The deny fold of deny set `set` (0-based) over an ingested batch, on the host: status[i] of
 * resource i (caller order) is what kv_deny_kernel writes for it, KV_STATUS_PASS / _FAIL / _ERROR /
 * _CPU, before match / exclude and the preconditions are applied. `n` must be the batch's
 * resource count. Diagnostics and tests; needs no GPU. */
int kv_batch_deny_fold(const kv_policyset* ps, const kv_batch* b, uint32_t set, uint8_t* status, uint64_t n);
/* validate.foreach rules evaluated on the device (KV_COMPILE_FOREACH): interned foreach sets
 * (list, entry preconditions, deny block), distinct lists, conditions with a variable operand and
 * element-scoped condition strings (keyed by list, text and resolver). Any may be NULL. */
int kv_policyset_foreach_sets(const kv_policyset* ps, uint32_t* sets, uint32_t* lists, uint32_t* conditions,
                              uint32_t* strings);
/* *set = 1 + the foreach set of rule `rule`, 0 for a rule that is not a device foreach rule
 * (kv_rule_deny_set is 0 for a foreach rule) */
int kv_rule_foreach_set(const kv_policyset* ps, uint32_t rule, uint32_t* set);
/* *on = 1 when rule `rule` is a device foreach rule whose entry carries a pattern
 * (KV_COMPILE_FOREACH_PATTERN), else 0 */
int kv_rule_foreach_pattern(const kv_policyset* ps, uint32_t rule, uint32_t* on);
/* Rules of several entries (KV_COMPILE_FOREACH_ENTRIES). A *chain* is the ordered list of the
 * foreach sets of a rule's entries, interned by that list. kv_policyset_foreach_chains: their
 * number. kv_rule_foreach_chain: *chain_plus_1 = 1 + the chain of rule `rule` and *n_entries its
 * entry count, both 0 for any other rule (kv_rule_foreach_set, kv_rule_foreach_pattern and
 * kv_rule_deny_set are 0 for a chain rule). kv_chain_entry_set: *set = the foreach set (0-based)
 * of entry `k` of chain `chain` (0-based); KV_E_RANGE past the end. */
int kv_policyset_foreach_chains(const kv_policyset* ps, uint32_t* chains);
int kv_rule_foreach_chain(const kv_policyset* ps, uint32_t rule, uint32_t* chain_plus_1, uint32_t* n_entries);
int kv_chain_entry_set(const kv_policyset* ps, uint32_t chain, uint32_t k, uint32_t* set);
/* The fold of chain `chain` (0-based) over an ingested batch, on the host: the twin of the entry
 * sets' kernels and kv_foreach_chain_kernel. status[i] of resource i (caller order) as
 * kv_batch_foreach_fold; entry[i] / elem[i] (each may be null) the deciding entry and the index of
 * the deciding element in that entry's list, 0xFFFFFFFF without one. Needs no GPU. KV_E_INVALID
 * when an entry of the chain carries a pattern. */
int kv_batch_foreach_chain_fold(const kv_policyset* ps, const kv_batch* b, uint32_t chain, uint8_t* status, uint32_t* entry,
                                uint32_t* elem, uint64_t n);
/* The text kv_result_foreach_message gives for resource `res` (caller order) of a chain where the
 * fold decides the pair, from the host fold alone: "validation failed in foreach rule for failed to
 * substitute variables in deny conditions: ..." for an ERROR (the first string that does not
 * resolve on the deciding element merged over what the entries before it leaked), "rule skipped"
 * for a SKIP; returns its length, 0 for any other status. Needs no GPU. KV_E_INVALID when an entry
 * of the chain carries a pattern. */
int kv_batch_foreach_chain_message(const kv_policyset* ps, const kv_batch* b, uint32_t chain, uint64_t res, char* buf,
                                   size_t cap);
/* (diagnostics) The per-batch foreach tables as the device receives them (sets, lists, element
 * rows, list states, pattern and chain tables, the gate's and the deny blocks' entries, outcome
 * ids and planes), each as a 64-bit count followed by its 32-bit words, in one buffer the caller
 * frees with kv_free_buffer. Needs no GPU. */
int kv_batch_foreach_tables(const kv_policyset* ps, const kv_batch* b, char** out, size_t* len);
/* *on = 1 when foreach set `set` (0-based) is a pattern set (its entry carries a pattern: no host
 * fold), else 0 */
int kv_foreach_set_pattern(const kv_policyset* ps, uint32_t set, uint32_t* on);
/* The foreach fold of foreach set `set` (0-based) over an ingested batch, on the host: the twin
 * of kv_foreach_elem_kernel and kv_foreach_fin_kernel. status[i] of resource i (caller order) is
 * KV_STATUS_PASS / _FAIL / _ERROR / _SKIP / _CPU before match / exclude and the rule's
 * preconditions are applied; elem[i] (may be NULL) the index of the deciding element in its list,
 * 0xFFFFFFFF without one. `n` must be the batch's resource count. Needs no GPU. KV_E_INVALID for
 * a set whose entry carries a pattern (KV_COMPILE_FOREACH_PATTERN): its elements are walked on the
 * device only. */
int kv_batch_foreach_fold(const kv_policyset* ps, const kv_batch* b, uint32_t set, uint8_t* status, uint32_t* elem,
                          uint64_t n);
int kv_rule_info_get(const kv_policyset* ps, uint32_t rule, kv_rule_info* out);

/* Ingest resources (JSON array or NDJSON of unstructured objects; numbers typed
 * like unstructured.UnmarshalJSON). ns_labels_json: {"<namespace>": {"k":"v"}}
 * (PolicyContext.NamespaceLabels per namespace) or NULL. */
int kv_ingest(const kv_policyset* ps, const char* resources_json, size_t len, const char* ns_labels_json,
              kv_batch** out, kv_error** err);
int kv_batch_info(const kv_batch* b, uint64_t* n_res, uint64_t* store_bytes);
/* bytes the batch's store crosses PCIe in (kv_validate's upload: the populated cells in their
 * 8-byte transfer form, row masks, values, resource headers, strings, match inputs); no
 * reference counterpart (the reference evaluates in the process that decoded the resource) */
int kv_batch_transfer_bytes(const kv_batch* b, uint64_t* bytes);
/* namespace table of a batch (first-seen order; index = scope of kv_result_scope_counts);
 * the name lives as long as the batch. Reference: resource.GetNamespace() keys the report
 * scope in buildPolicyResults (pkg/kyverno/apply/report.go:80-87). */
int kv_batch_namespaces(const kv_batch* b, uint32_t* n);
const char* kv_batch_namespace(const kv_batch* b, uint32_t i);

/* Evaluate every (resource, rule) pair on HIP device `device`.
 * ctx_json: {"admission": {"roles":[], "clusterRoles":[], "groups":[], "username":""},
 *            "excludeGroupRole": []}  (PolicyContext.AdmissionInfo / ExcludeGroupRole) or NULL. */
int kv_validate(const kv_policyset* ps, const kv_batch* b, const char* ctx_json, int device, uint32_t mode,
                kv_result** out, kv_error** err);

/* Evaluate on several devices (SURVEY.md §8b "Threading"): the batch's resources are
 * split into contiguous ranges [k*N/G, (k+1)*N/G) (cut at 64-resource boundaries)
 * over the G devices of device_mask (bit d = HIP device d), one host thread + HIP
 * stream per device, the policy set replicated; per-rule counts (and per-scope
 * counts with KV_MODE_SCOPES) are summed over the devices by one RCCL all-reduce
 * (ncclUint64, ncclSum; communicators created per session). Statuses and error
 * records come back in resource order in one result. Callers: the background
 * scan (pkg/policy/apply.go:72) and kyverno apply (pkg/kyverno/apply/apply_command.go:270-310). */
int kv_validate_devices(const kv_policyset* ps, const kv_batch* b, const char* ctx_json, uint32_t device_mask,
                        uint32_t mode, kv_result** out, kv_error** err);

/* status[rule * n_res + res] (rule-major). The statuses of a specialized pass cross PCIe in a
 * transfer form (the 256-resource segments the pass wrote, 4 bits a status; the others NOMATCH);
 * the first call with a non-NULL `status` builds the dense matrix on the host threads (C3 1.25 M x
 * 1 973: ~60 ms) and later calls return it. status = NULL: dimensions only, nothing built. */
int kv_result_status(const kv_result* r, const uint8_t** status, uint64_t* n_rules, uint64_t* n_res);
/* counts[rule * 8 + status] */
int kv_result_counts(const kv_result* r, const int64_t** counts);
/* Page-lock `bytes` of host memory for the library's store and result arrays up front (once per
 * process; a later call only reports whether the reserve is at least that large), so the ingest of
 * a process's first batch and its first results find page-locked memory instead of pinning it
 * then. 0 on success, KV_E_DEVICE without a device or when the host refuses the memory. */
int kv_host_reserve(uint64_t bytes);
/* Device buffers released by batches, results and sessions are kept per device and handed to the
 * next allocation of a similar size (a released buffer is reused only after the work queued before
 * its release has finished). kv_device_pool_limit sets how many bytes are kept per device (default
 * 32 GiB; 0 keeps none); kv_device_trim frees what device `device` keeps now, e.g. before another
 * allocator in the process (torch) needs the memory. No reference counterpart (Go frees nothing
 * on a device). 0 on success, KV_E_DEVICE for a bad device. */
int kv_device_pool_limit(uint64_t bytes);
int kv_device_trim(int device);
/* phase i of the kv_validate that produced r: its name ("upload", "setup", "pass", "host_alloc",
 * "status_d2h", "records_count", "records_scatter_d2h", ...) and wall-clock milliseconds;
 * KV_E_RANGE past the last phase. Diagnostics of the host boundary (no reference counterpart).
 * "precond" (policy sets with device-evaluated preconditions): the HIP-event time of the
 * precondition gate's kernel, which runs once per batch when the batch is uploaded. "deny"
 * (policy sets with device deny rules): the same for the deny fold's kernel. "foreach" (device
 * foreach rules): the same for the foreach fold's two kernels and the clearing of their keys. */
int kv_result_phase(const kv_result* r, uint32_t i, const char** name, double* ms);
/* counts[(scope * n_rules + rule) * 8 + status] (KV_MODE_SCOPES) */
int kv_result_scope_counts(const kv_result* r, const int64_t** counts, uint32_t* n_scopes);
/* failing path of a FAIL pair, e.g. "/spec/containers/0/image/" (needs KV_MODE_ERRORS);
 * returns the string length, or a negative code. */
int kv_result_path(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap);
/* raw error record: kind (validate.go/anchor.go error form) and anchor-wrap flags */
int kv_result_error(const kv_result* r, uint32_t rule, uint64_t res, uint32_t* kind, uint32_t* flags);
/* err.Error() of the PatternError behind a FAIL / ERROR / SKIP pair — the SKIP
 * message and the "execution error: %s" operand of the ERROR message
 * (pkg/engine/validation.go:421-439,510-527; error forms of
 * pkg/engine/validate/validate.go:62-172 and pkg/engine/anchor/anchor.go:61-261).
 * The caller passes the resource document (JSON) it ingested, from which the
 * Go '%v' / %T operands are formatted. Returns the message length, KV_E_INVALID
 * for other statuses or constant (compile-time) statuses, KV_E_PARSE for bad JSON. */
int kv_result_error_message(const kv_result* r, uint32_t rule, uint64_t res, const char* resource_json, size_t len,
                            char* buf, size_t cap);

/* Pattern variables: when rule `rule` is ERROR on `res` because
 * substituting the `{{request.object...}}` variables of its pattern failed, writes the
 * RuleResponse message "variable substitution failed: <error>" (pkg/engine/validation.go:
 * 181-189, the reference's processValidationRule -> substitutePatterns) and returns its
 * length; 0 when the pair's status has another cause. */
int kv_result_subst_error(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap);

/* Preconditions: when rule `rule` is SKIP on `res` because its preconditions do not hold
 * (pkg/engine/validation.go:175-184), writes the RuleResponse message "preconditions not met"
 * and returns its length; 0 when the status has another cause (a conditional-anchor SKIP of the
 * pattern). Negative codes as kv_result_subst_error. */
int kv_result_precond_message(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap);

/* Deny rules (KV_COMPILE_DENY): when rule `rule` is ERROR on `res` because a variable of its
 * deny conditions does not resolve (pkg/engine/validation.go:299-304), writes the RuleResponse
 * message "failed to substitute variables in deny conditions: <error>" and returns its length; 0
 * when the status has another cause or the rule is not a device deny rule. With several
 * unresolved strings the error is the first in document order (the reference ranges over a Go
 * map there: its order is not fixed). Negative codes as kv_result_subst_error. The PASS and FAIL
 * messages are formed by the caller from kv_rule_info. */
int kv_result_deny_message(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap);

/* Foreach rules (KV_COMPILE_FOREACH). kv_result_foreach_element: *index = the index in its list
 * of the element that decided a FAIL or ERROR pair of a device foreach rule (the caller
 * substitutes the rule's message with it as `element`: "validation failed in foreach rule for " +
 * message), 0xFFFFFFFF for every other pair. kv_result_foreach_message: for an
 * ERROR pair "validation failed in foreach rule for failed to substitute variables in deny
 * conditions: <error>" (the first unresolved string of the deciding element, in the order of
 * kv_result_deny_message); for a SKIP pair the fold decided "rule skipped" (a SKIP of the rule's
 * own preconditions is kv_result_precond_message's); returns the length, 0 for any other cause
 * (kv_result_deny_message is 0 for foreach rules). Negative codes as kv_result_subst_error. */
int kv_result_foreach_element(const kv_result* r, uint32_t rule, uint64_t res, uint32_t* index);
int kv_result_foreach_message(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap);
/* Rules of several entries (KV_COMPILE_FOREACH_ENTRIES). A result fetched with statuses carries
 * a 4-byte key per (chain, resource): the deciding entry, its element and the code.
 * kv_result_foreach_entry: *entry = the position of the entry that decided a FAIL or ERROR pair
 * (0 for a rule of one entry), 0xFFFFFFFF for every other pair; kv_result_foreach_element then
 * gives the index within that entry's list, and kv_result_foreach_message, _path and
 * _error_message answer through the deciding entry's set (the ERROR text of a deny entry names
 * the first string that does not resolve on the merged element). */
int kv_result_foreach_entry(const kv_result* r, uint32_t rule, uint64_t res, uint32_t* entry);
/* Pattern entries (KV_COMPILE_FOREACH_PATTERN). A result fetched with statuses carries, per
 * pattern set and resource, the reduction key (the deciding element and its code) and the deciding
 * element's 8-byte error record; kv_result_foreach_element reads the key for these rules, and
 * kv_result_foreach_message gives only "rule skipped" for them.
 * kv_result_foreach_path: the failing path of a FAIL pair, relative to the deciding element
 * ("/image/", "/ports/1/containerPort/"); returns its length, KV_E_INVALID for any other pair.
 * kv_result_foreach_error_message: err.Error() of the deciding element's PatternError (FAIL and
 * ERROR pairs), formatted from `element_json`, the caller's document of that element, with every
 * number typed float64 as the reference's element is ("8.08e+06", "float64"); returns its length,
 * KV_E_INVALID for any other pair, KV_E_PARSE for bad JSON. The caller composes the RuleResponse
 * message: "validation failed in foreach rule for " + buildErrorMessage. */
int kv_result_foreach_path(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap);
int kv_result_foreach_error_message(const kv_result* r, uint32_t rule, uint64_t res, const char* element_json, size_t len,
                                    char* buf, size_t cap);
/* anyPattern entries (KV_COMPILE_FOREACH_ANYPATTERN). kv_rule_foreach_anypattern: *n_alts = the
 * alternative count of a device foreach rule whose one entry carries an anyPattern, 0 for every
 * other rule (kv_rule_foreach_pattern is 0 for it). kv_foreach_set_alternatives: the same for
 * foreach set `set` (0-based; the entries of a chain), 0 for a set that is no any set. A result
 * fetched with statuses carries, per (any set, resource), the reduction key, a code word (4 bits
 * per alternative: its status on the deciding element) and one 8-byte record per alternative.
 * kv_result_foreach_alt: for a FAIL pair decided by an anyPattern entry, *status = the status of
 * alternative `alt` on the deciding element (the FAIL, ERROR or SKIP status code) and, for FAIL, its
 * failing path relative to the element in buf; returns the path's length (0 without one),
 * KV_E_INVALID for any other pair, KV_E_RANGE for an alternative the set does not have.
 * kv_result_foreach_alt_error_message: err.Error() of that alternative's PatternError, formatted
 * from `element_json` with float64 typing as kv_result_foreach_error_message. The caller composes
 * buildAnyPatternErrorMessage: per alternative "Rule <name>[<alt>] failed at path <path>." where
 * the path is not empty, else "Rule <name>[<alt>] failed: <error>." (INTEGRATION.md).
 * kv_result_foreach_path and kv_result_foreach_error_message are KV_E_INVALID for such a pair, and
 * kv_result_failures keeps KV_PATH_NONE. */
int kv_rule_foreach_anypattern(const kv_policyset* ps, uint32_t rule, uint32_t* n_alts);
int kv_foreach_set_alternatives(const kv_policyset* ps, uint32_t set, uint32_t* n);
int kv_result_foreach_alt(const kv_result* r, uint32_t rule, uint64_t res, uint32_t alt, uint32_t* status, char* buf,
                          size_t cap);
int kv_result_foreach_alt_error_message(const kv_result* r, uint32_t rule, uint64_t res, uint32_t alt,
                                        const char* element_json, size_t len, char* buf, size_t cap);
/* Pattern variables in entries (KV_COMPILE_FOREACH_PATVARS). kv_rule_foreach_patvars: *on = 1
 * for a device foreach rule with an entry whose pattern or alternatives hold variable strings,
 * else 0. kv_result_foreach_subst_error: for an ERROR pair whose deciding element failed the
 * substitution of its entry's pattern, "validation failed in foreach rule for variable
 * substitution failed: <err>" (the RuleResponse message), recomputed on the host from that
 * element's outcome row; returns its length, 0 for every other pair (an ERROR the pattern walk
 * gave is kv_result_foreach_error_message's). kv_result_foreach_error_message and
 * kv_result_foreach_alt_error_message render the deciding element's substituted value at a
 * dynamic leaf. kv_batch_foreach_subst (diagnostics and tests, as kv_batch_foreach_fold and
 * kv_batch_foreach_chain_fold: not part of the evaluation path): the substitution verdict of element `elem` of caller
 * resource `res` under the pattern strings of foreach set `set` on the host (no GPU; the function
 * the kernels run): *code = 0, the ERROR or the CPU status code, and for ERROR the <err> text in
 * buf; returns its length, KV_E_INVALID for a set without variable strings, KV_E_RANGE for an
 * element the resource's list does not have. */
int kv_rule_foreach_patvars(const kv_policyset* ps, uint32_t rule, uint32_t* on);
int kv_result_foreach_subst_error(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap);
int kv_batch_foreach_subst(const kv_policyset* ps, const kv_batch* b, uint32_t set, uint64_t res, uint32_t elem,
                           uint32_t* code, char* buf, size_t cap);
double kv_result_kernel_ms(const kv_result* r);

/* Bulk export of the failing pairs (KV_MODE_ERRORS): every FAIL / ERROR / SKIP pair,
 * rule-major and in resource order: pair i = (rule[i], res[i]); path_id[i] names the
 * failing path of a FAIL pair (KV_PATH_NONE for ERROR / SKIP), rendered once per
 * distinct path by kv_path_string (e.g. "/spec/containers/0/image/"; ids numbered by first
 * appearance in the returned order). The arrays and
 * strings live as long as the result. This is what a Go caller builds
 * RuleResponse.Message from without one call per pair (validation.go:510-547). */
enum { KV_PATH_NONE = 0xFFFFFFFFu };
int kv_result_failures(const kv_result* r, uint64_t* n, const uint32_t** rule, const uint64_t** res,
                       const uint32_t** path_id);
const char* kv_path_string(const kv_result* r, uint32_t path_id);

/* Benchmark entry: device-resident inputs, `iters` timed launches on one stream
 * bracketed by HIP events. Returns mean kernel milliseconds per pass over all
 * rules of the batch. */
int kv_bench(const kv_policyset* ps, const kv_batch* b, const char* ctx_json, int device, uint32_t mode, int warmup,
             int iters, double* ms_per_iter, kv_error** err);

/* Session: device-resident inputs and output buffers allocated once
 * (kv_session_create, untimed); kv_session_run enqueues `iters` passes on the
 * session's stream and waits for them, returning the HIP-event time of the
 * passes (ms, total). For benchmarks and repeated background scans. */
typedef struct kv_session kv_session;
int kv_session_create(const kv_policyset* ps, const kv_batch* b, const char* ctx_json, int device, uint32_t mode,
                      kv_session** out, kv_error** err);
/* multi-device session (see kv_validate_devices); kv_session_counts / _scope_counts
 * return the RCCL-reduced totals, kv_session_fetch the last pass as a result */
int kv_session_create_devices(const kv_policyset* ps, const kv_batch* b, const char* ctx_json, uint32_t device_mask,
                              uint32_t mode, kv_session** out, kv_error** err);
int kv_session_parts(const kv_session* s, uint32_t* n_parts);
int kv_session_fetch(kv_session* s, kv_result** out, kv_error** err);
int kv_session_run(kv_session* s, int iters, double* event_ms, kv_error** err);
int kv_session_counts(kv_session* s, int64_t* counts /* [n_rules][8], last pass */);
int kv_session_scope_counts(kv_session* s, int64_t* counts /* [n_scopes][n_rules][8], last pass */);
void kv_free_session(kv_session* s);
/* Multi-device session assembled from per-device batches: each part's resources are
 * ingested on their own (a background-scan worker per GPU, or one host feeding G devices
 * without holding the whole node's batch; pkg/policy/policy_controller.go:453-454 ->
 * pkg/policy/apply.go:72). kv_session_create_parts opens a session of n_parts parts;
 * kv_session_attach_part uploads batch b to HIP device `device` as part `part` — the
 * session keeps only the device copy, so the caller may free b right after. When the last
 * part is attached the scopes become the sorted union of the parts' namespaces
 * (kv_session_scopes / kv_session_scope_name) and the RCCL communicator is created (distinct
 * devices); run / counts / scope_counts then work as for kv_session_create_devices
 * (KV_E_DEVICE before that). kv_session_fetch is not available (no host batch). */
int kv_session_create_parts(const kv_policyset* ps, const char* ctx_json, uint32_t mode, uint32_t n_parts,
                            kv_session** out, kv_error** err);
int kv_session_attach_part(kv_session* s, uint32_t part, const kv_batch* b, int device, kv_error** err);
/* scope table of a session (batch namespaces; the union of the parts' for a parts session) */
int kv_session_scopes(const kv_session* s, uint32_t* n_scopes);
const char* kv_session_scope_name(const kv_session* s, uint32_t i);
/* ranks of the session's RCCL communicator (0: counts summed on the host — one part, or
 * logical parts of one device) and the HIP-event ms of each part's last kv_session_run */
int kv_session_rccl_ranks(const kv_session* s, int* ranks);
int kv_session_part_ms(const kv_session* s, double* ms /* [n_parts] */);
/* status-matrix bytes the last pass wrote: the specialized kernels write a rule's statuses of a
 * 256-resource workgroup only when one of them is not NOMATCH and flag the segment (an unwritten
 * segment is filled with NOMATCH at fetch); the bytecode engine writes the whole matrix. The
 * output bytes of a pass for the roofline accounting (no reference counterpart). */
int kv_session_status_bytes(kv_session* s, uint64_t* bytes);

/* Synthetic resource generator for the benchmark configs:
 * kind_mix 0 = Pods; 1 = Pods/Deployments/Services 60/25/15 (64 namespaces each);
 * 2 = the mixed kinds over 1 000 namespaces (C3). Returns NDJSON
 * (free with kv_free_buffer). */
int kv_synth(uint64_t seed, uint64_t n, uint32_t kind_mix, char** json_out, size_t* len);
/* resources [first, first + n) of the same stream (a rank's contiguous shard) */
int kv_synth_range(uint64_t seed, uint64_t first, uint64_t n, uint32_t kind_mix, char** json_out, size_t* len);

void kv_free_policyset(kv_policyset* ps);
void kv_free_batch(kv_batch* b);
void kv_free_result(kv_result* r);
void kv_free_error(kv_error* e);
void kv_free_buffer(char* p);

#ifdef __cplusplus
}
#endif
#endif /* KVGPU_H */
