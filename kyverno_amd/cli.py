"""`kyverno apply` / `kyverno test` front end over the batch engine.

Mirrors the reference CLI for validate rules:

* ``apply POLICY... -r RESOURCE... [--policy-report]`` — ``applyCommandHelper`` +
  ``printReportOrViolation`` (pkg/kyverno/apply/apply_command.go:147-381):
  policies loaded and mutated (defaults + autogen, ``common.MutatePolices``,
  pkg/kyverno/common/common.go:429-444 → ``kyverno_amd.autogen``), resources
  loaded with the unstructured number typing and namespace "default"
  (pkg/kyverno/common/fetch.go:251-279), every (policy, resource) pair evaluated,
  counted with ``ProcessValidateEngineResponse`` (common.go:703-766), violations
  printed, summary line printed, exit status 1 on fail/error.
* ``test DIR`` — ``kyverno test`` over a ``test.yaml`` (pkg/kyverno/test/
  test_command.go:347-494): each expected result is looked up by policy, rule
  (with the ``autogen-`` / ``autogen-cronjob-`` fallback) and resource.

Evaluation runs on the GPU through the C ABI (``kyverno_amd.batch``): one
``kv_validate`` over the whole (rule × resource) cross product instead of the
reference's per-pair ``engine.Validate`` loop (apply_command.go:270-310). Rules
the device does not evaluate (variables other than ``request.object`` paths,
context, deny, foreach, preconditions outside the device forms — ``KV_ROUTE_CPU``) are reported as
routed to the reference engine and not counted; preconditions of the device forms (any / all of
Equals, In, GreaterThan ... conditions on ``request.object`` paths) are evaluated with the rule: a
pair whose preconditions do not hold is `skip`, "preconditions not met"; a Go host runs them through ``engine.Validate``.
``--device-deny`` (``evaluate(deny=True)``, ``KV_COMPILE_DENY``) also evaluates ``validate.deny`` rules
whose conditions are of those forms on the device, with the messages of ``validateDeny``.
``--device-foreach`` (``evaluate(foreach=True)``, ``KV_COMPILE_FOREACH``) does the same for single-entry
``validate.foreach`` rules with a ``deny`` block, with the messages of ``validateForEach``;
``--device-foreach-pattern`` (``evaluate(foreach_pattern=True)``, ``KV_COMPILE_FOREACH_PATTERN``; implies
``--device-foreach``) also for entries that carry a ``pattern``; ``--device-foreach-entries``
(``evaluate(foreach_entries=True)``, ``KV_COMPILE_FOREACH_ENTRIES``; implies ``--device-foreach``) also for
rules of several entries; ``--device-foreach-anypattern`` (``evaluate(foreach_anypattern=True)``,
``KV_COMPILE_FOREACH_ANYPATTERN``; implies ``--device-foreach-pattern`` and ``--device-foreach``) also for
entries that carry an ``anyPattern``, with the message of ``buildAnyPatternErrorMessage``;
``--device-foreach-patvars`` (``evaluate(foreach_patvars=True)``, ``KV_COMPILE_FOREACH_PATVARS``; implies
``--device-foreach-pattern`` and ``--device-foreach``) also for entries whose pattern or alternatives hold
``{{element...}}`` / ``{{request.object...}}`` variables, with the element's "variable substitution failed" error.

    python -m kyverno_amd apply policy.yaml -r pods.yaml [--policy-report] [--device N] [--device-deny] [--device-foreach]
        [--device-foreach-pattern] [--device-foreach-entries] [--device-foreach-anypattern] [--device-foreach-patvars]
    python -m kyverno_amd test test/cli/test/simple
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
from dataclasses import dataclass, field

import numpy as np

from . import autogen, msgvars, yamlio

PASS, FAIL, WARN, ERROR, SKIP, NOMATCH, CPU = range(7)  # kv status codes (include/kvgpu.h)
ROUTE_NORESPONSE = 2  # KV_ROUTE_NORESPONSE: not a validate rule, never in the validate response
REPORT_STATUS = {PASS: "pass", FAIL: "fail", WARN: "warn", ERROR: "error", SKIP: "skip"}
DIVIDER = "-" * 70
# variables.RegexVariables (pkg/engine/variables/vars.go:20)
_REGEX_VARIABLES = re.compile(r"^\{\{[^{}]*\}\}|[^\\]\{\{[^{}]*\}\}")


# ---------------------------------------------------------------- loading


def _yaml_files(path: str) -> list[str]:
    if os.path.isdir(path):
        out = []
        for root, _, files in sorted(os.walk(path)):
            out += [os.path.join(root, f) for f in sorted(files) if f.endswith((".yaml", ".yml", ".json"))]
        return out
    return [path]


def load_policies(paths: list[str]) -> list[dict]:
    """common.GetPolicies (pkg/kyverno/common/common.go:83-168): files or directories."""
    out = []
    for p in paths:
        for f in _yaml_files(p):
            out += [yamlio.to_go_json_obj(x) for x in yamlio.load_policies_file(f)]
    return out


def load_resources(paths: list[str]) -> list[dict]:
    """whenClusterIsFalse → GetResource (fetch.go:110-190): documents without a kind are dropped."""
    out = []
    for p in paths:
        for f in _yaml_files(p):
            out += [yamlio.to_go_json_obj(x) for x in yamlio.load_resources_file(f)]
    return out


def has_unset_variables(policy: dict) -> bool:
    """common.HasVariables + RemoveDuplicateAndObjectVariables (common.go:76-80, :298-311): a policy
    with a `{{ }}` variable that is not request.object / element needs --set / --values-file values
    and is skipped by `apply` (apply_command.go:283-293)."""
    raw = json.dumps(policy, separators=(",", ":"), ensure_ascii=False)
    for m in _REGEX_VARIABLES.finditer(raw):
        v = m.group(0)
        if "request.object" not in v and "element" not in v:
            return True
    return False


# ---------------------------------------------------------------- evaluation


@dataclass
class Evaluation:
    """Per-(rule, resource) statuses of one evaluation of the mutated policies."""
    policies: list          # mutated policies, as evaluated
    resources: list
    rules: list             # batch.Rule per compiled rule (policy order)
    status: np.ndarray      # u8 [n_rules][n_res]
    paths: dict = field(default_factory=dict)   # (rule, res) -> failing path (FAIL pairs)
    errors: dict = field(default_factory=dict)  # (rule, res) -> err.Error() of ERROR / SKIP pairs
    subst: dict = field(default_factory=dict)   # (rule, res) -> message of a pattern-variable substitution ERROR
    precond: dict = field(default_factory=dict)  # (rule, res) -> message of a SKIP decided by the preconditions
    deny: dict = field(default_factory=dict)    # (rule, res) -> message of an ERROR of a deny rule's substitution
    foreach: dict = field(default_factory=dict)  # (rule, res) -> message of an ERROR / SKIP of a foreach rule
    foreach_elem: dict = field(default_factory=dict)  # (rule, res) -> index of the deciding element (FAIL)
    foreach_entry: dict = field(default_factory=dict)  # (rule, res) -> the deciding entry (rules of several entries)
    foreach_path: dict = field(default_factory=dict)  # (rule, res) -> failing path in the deciding element (pattern entries)
    foreach_err: dict = field(default_factory=dict)   # (rule, res) -> pattern error of the deciding element (pattern entries, ERROR)
    foreach_alts: dict = field(default_factory=dict)  # (rule, res) -> [(status, path, error text)] per alternative (anyPattern entries, FAIL)
    anypattern: dict = field(default_factory=dict)  # (rule, res) -> [(status, path)] per pattern
    warnings: list = field(default_factory=list)    # host-side limits met while rendering messages

    def policy_rules(self, pi: int) -> list:
        return [r for r in self.rules if r.policy == pi]


def evaluate(policies: list[dict], resources: list[dict], device: int = 0, messages: bool = True,
             namespace_labels: dict | None = None, specialize: bool = False, gpus: int = 1,
             deny: bool = False, foreach: bool = False, foreach_pattern: bool = False,
             foreach_entries: bool = False, foreach_anypattern: bool = False,
             foreach_patvars: bool = False) -> Evaluation:
    """All (rule, resource) pairs on the GPU (``kv_compile`` → ``kv_ingest`` → ``kv_validate``).
    ``specialize`` selects the per-policy-set specialized kernels (worth their hiprtc compile on
    large batches) over the bytecode interpreter; both write the same statuses and error records.
    ``gpus`` > 1 shards the resources over devices [device, device + gpus) (kv_validate_devices).
    ``deny`` evaluates ``validate.deny`` rules of the device forms on the GPU (``KV_COMPILE_DENY``)
    instead of routing them to the reference engine; ``foreach`` does the same for
    ``validate.foreach`` rules (``KV_COMPILE_FOREACH``), ``foreach_pattern`` (which implies
    ``foreach``) also for entries that carry a ``pattern`` (``KV_COMPILE_FOREACH_PATTERN``),
    ``foreach_entries`` (which implies ``foreach`` too) also for rules of several entries
    (``KV_COMPILE_FOREACH_ENTRIES``), ``foreach_anypattern`` (which implies ``foreach_pattern`` and
    ``foreach``) also for entries that carry an ``anyPattern`` (``KV_COMPILE_FOREACH_ANYPATTERN``),
    ``foreach_patvars`` (which implies ``foreach_pattern`` and ``foreach``) also for entries whose
    pattern or alternatives hold ``{{element...}}`` / ``{{request.object...}}`` variables
    (``KV_COMPILE_FOREACH_PATVARS``)."""
    from . import batch

    foreach_pattern = foreach_pattern or foreach_anypattern or foreach_patvars
    ps = batch.PolicySet(policies, specialize=specialize, deny=deny,
                         foreach=foreach or foreach_pattern or foreach_entries,
                         foreach_pattern=foreach_pattern, foreach_entries=foreach_entries,
                         foreach_anypattern=foreach_anypattern, foreach_patvars=foreach_patvars)
    b = batch.Batch(ps, resources, namespace_labels)
    mask = ((1 << gpus) - 1) << device if gpus > 1 else None
    r = batch.validate(ps, b, device=device, device_mask=mask)
    ev = Evaluation(policies, resources, ps.rules, r.status)
    if messages:
        for ri, res in zip(*np.nonzero(r.status == FAIL)):
            if ps.rules[ri].foreach:  # (no failing path either: the deciding element instead)
                ev.foreach_elem[(int(ri), int(res))] = r.foreach_element(int(ri), int(res))
                if getattr(ps.rules[ri], "foreach_entries", 0):  # (several entries: which one decided)
                    ev.foreach_entry[(int(ri), int(res))] = r.foreach_entry(int(ri), int(res))
                if _pattern_entry(ev, ps.rules[ri], int(res)):  # (a pattern entry: the path inside that element)
                    ev.foreach_path[(int(ri), int(res))] = r.foreach_path(int(ri), int(res))
                if _any_entry(ev, ps.rules[ri], int(res)):  # (an anyPattern entry: every alternative's outcome on it)
                    ev.foreach_alts[(int(ri), int(res))] = _foreach_alts(ev, ps.rules[ri], r, int(res))
            elif not ps.rules[ri].any_pattern and not ps.rules[ri].deny:  # (a deny FAIL has no failing path)
                ev.paths[(int(ri), int(res))] = r.path(int(ri), int(res))
        collect_errors(ev, ps, r, resources)
        _evaluate_anypatterns(ev, device, specialize, namespace_labels)
    return ev


def collect_errors(ev: Evaluation, ps, r, resources: list) -> None:
    """Messages of the ERROR / SKIP pairs: pattern-variable substitution errors and preconditions
    that do not hold (whole message), else the pattern error's err.Error() (pattern rules; anyPattern rules render per pattern)."""
    for ri, res in zip(*np.nonzero((r.status == ERROR) | (r.status == SKIP))):
        key = (int(ri), int(res))
        if r.status[ri, res] == ERROR:
            m = r.subst_error(*key)
            if m is not None:
                ev.subst[key] = m
                continue
            m = r.deny_message(*key)
            if m is not None:
                ev.deny[key] = m
                continue
            if getattr(ps.rules[ri], "foreach_patvars", False):
                # the deciding element failed the substitution of its entry's pattern: the whole message
                m = r.foreach_subst_error(*key)
                if m is not None:
                    ev.subst[key] = m
                    continue
        else:
            m = r.precond_message(*key)
            if m is not None:
                ev.precond[key] = m
                continue
        if getattr(ps.rules[ri], "foreach_entries", 0) and r.status[ri, res] == ERROR:
            ev.foreach_entry[key] = r.foreach_entry(*key)
        if r.status[ri, res] == ERROR and _pattern_entry(ev, ps.rules[ri], key[1]):
            # a pattern entry: the pattern error of the deciding element, formatted from that element
            ev.foreach_elem[key] = r.foreach_element(*key)
            el = _foreach_element(ev, ps.rules[ri], key[1])
            m = r.foreach_error_message(key[0], key[1], el) if el is not None else None
            if m is not None:
                ev.foreach_err[key] = m
            continue
        if getattr(ps.rules[ri], "foreach", False):
            m = r.foreach_message(*key)
            if m is not None:
                ev.foreach[key] = m
            continue
        if not ps.rules[ri].any_pattern:
            m = r.error_message(int(ri), int(res), resources[int(res)])
            if m is not None:
                ev.errors[key] = m


def _evaluate_anypatterns(ev: Evaluation, device: int, specialize: bool = False,
                          namespace_labels: dict | None = None) -> None:
    """Per-pattern outcomes of anyPattern rules, for the pass index and the failure message of
    validatePatterns (pkg/engine/validation.go:446-484): every pattern of the rule is compiled as a
    pattern rule of its own (same match/exclude) and run on the device over the resources where
    the anyPattern rule passed or failed."""
    from . import batch

    todo = [(r, np.nonzero((ev.status[r.index] == PASS) | (ev.status[r.index] == FAIL))[0])
            for r in ev.rules if r.any_pattern]
    todo = [(r, idx) for r, idx in todo if len(idx)]
    if not todo:
        return
    for rule, idx in todo:
        src = ev.policies[rule.policy]
        rdoc = next(x for x in src["spec"]["rules"] if x.get("name") == rule.name)
        pats = rdoc["validate"]["anyPattern"]
        sub_rules = []
        for j, p in enumerate(pats):
            sr = {k: v for k, v in rdoc.items() if k != "validate"}
            sr["name"] = f"{rule.name}[{j}]"
            sr["validate"] = {"message": rdoc["validate"].get("message", ""), "pattern": p}
            sub_rules.append(sr)
        sub = {"apiVersion": src.get("apiVersion", "kyverno.io/v1"), "kind": src.get("kind", "ClusterPolicy"),
               "metadata": src.get("metadata", {}), "spec": {"rules": sub_rules}}
        ps = batch.PolicySet([sub], specialize=specialize)
        ress = [ev.resources[i] for i in idx]
        b = batch.Batch(ps, ress, namespace_labels)
        r = batch.validate(ps, b, device=device)
        for k, res in enumerate(idx):
            outs = []
            for j in range(len(pats)):
                st = int(r.status[j, k])
                if st == FAIL:
                    outs.append((st, r.path(j, k)))
                elif st in (ERROR, SKIP):  # PatternError with an empty path: its text
                    outs.append((st, r.error_message(j, k, ress[k])))
                else:
                    outs.append((st, None))
            ev.anypattern[(rule.index, int(res))] = outs


# ---------------------------------------------------------------- messages


def _with_dot(s: str) -> str:
    return s if s.endswith(".") else s + "."


def _message(ev: Evaluation, rule, res: int, element: dict | None = None) -> str:
    """The rule's message after SubstituteAll (msgvars), with ``element`` in the context of a foreach
    entry. A JMESPath form the host does not evaluate leaves the message as written and is reported
    in ``ev.warnings``; a form on which the reference panics raises ``msgvars.MessageVariableError``."""
    try:
        return msgvars.substitute_message(rule.message, ev.resources[res], element)
    except msgvars.UnsupportedMessageVariable as e:
        w = f"rule {rule.name}: message variables not rendered: {e}"
        if w not in ev.warnings:
            ev.warnings.append(w)
        return rule.message


def _foreach_entries(ev: Evaluation, rule) -> list:
    """The entries of a foreach rule, as written."""
    src = ev.policies[rule.policy]
    rdoc = next(x for x in src["spec"]["rules"] if x.get("name") == rule.name)
    return rdoc["validate"]["foreach"]


def _deciding_entry(ev: Evaluation, rule, res: int) -> int | None:
    """The position of the entry that decided the pair: 0 for a rule of one entry, what the device
    reported for a rule of several (None: no entry decided)."""
    if not getattr(rule, "foreach_entries", 0):
        return 0
    return ev.foreach_entry.get((rule.index, res))


def _pattern_entry(ev: Evaluation, rule, res: int) -> bool:
    """The pair of a device foreach rule was decided by an entry that carries a pattern."""
    if getattr(rule, "foreach_pattern", False):
        return True
    if not getattr(rule, "foreach_entries", 0):
        return False
    k = _deciding_entry(ev, rule, res)
    return k is not None and "pattern" in _foreach_entries(ev, rule)[k]


def _any_entry(ev: Evaluation, rule, res: int) -> bool:
    """The pair of a device foreach rule was decided by an entry that carries an anyPattern."""
    if getattr(rule, "foreach_anypattern", 0):
        return True
    if not getattr(rule, "foreach_entries", 0):
        return False
    k = _deciding_entry(ev, rule, res)
    return k is not None and "anyPattern" in _foreach_entries(ev, rule)[k]


def _foreach_alts(ev: Evaluation, rule, r, res: int) -> list:
    """Per alternative of the deciding anyPattern entry of a FAIL pair, on the deciding element:
    (status, failing path, err.Error() where the path is empty); None for one the device did not
    report."""
    k = _deciding_entry(ev, rule, res)
    el = _foreach_element(ev, rule, res)
    outs = []
    for a in range(len(_foreach_entries(ev, rule)[k]["anyPattern"])):
        o = r.foreach_alt(rule.index, res, a)
        if o is None:
            outs.append(None)
            continue
        st, path = o
        text = None
        if not path and el is not None:
            text = r.foreach_alt_error_message(rule.index, res, a, el)
        outs.append((st, path, text))
    return outs


def _entry_list(entry: dict, resource) -> list | None:
    """evaluateList of one entry: None where the query fails, a map is a one-element list."""
    try:
        lst = msgvars.query(entry["list"], {"request": {"object": resource}})
    except msgvars.MessageVariableNotFound:
        return None
    return [lst] if isinstance(lst, dict) else lst


def merge_maps(base, over):
    """The JSON merge of two documents without nulls (jsonpatch.MergeMergePatches, as AddJSON uses
    it): two maps merge key by key, anything else replaces what was there."""
    if not (isinstance(base, dict) and isinstance(over, dict)):
        return over
    out = dict(base)
    for k, v in over.items():
        out[k] = merge_maps(out[k], v) if k in out else v
    return out


def foreach_leak_base(entries: list, resource, k: int):
    """What the reference's context holds as ``element`` when entry ``k`` of a foreach rule starts
    (validateForEach: the checkpoint of an entry is taken with the last element of the entry before
    it still merged in): the last elements of the lists of entries 0 .. k-1, merged in order; an
    entry whose list query fails or gives no element adds nothing. None: nothing leaked."""
    base = None
    for e in entries[:k]:
        lst = _entry_list(e, resource)
        if isinstance(lst, list) and lst and isinstance(lst[-1], dict):
            base = lst[-1] if base is None else merge_maps(base, lst[-1])
    return base


def _foreach_element(ev: Evaluation, rule, res: int, merged: bool = False):
    """The deciding element of a FAIL pair of a device foreach rule: the deciding entry's list
    evaluated on the resource (a map is a one-element list), at the index the device reported.
    ``merged``: as the variables of that entry see it, over what the entries before it leaked."""
    idx = ev.foreach_elem.get((rule.index, res))
    k = _deciding_entry(ev, rule, res)
    if k is None:
        return None
    entries = _foreach_entries(ev, rule)
    lst = _entry_list(entries[k], ev.resources[res])
    el = lst[idx] if idx is not None and isinstance(lst, list) and idx < len(lst) else None
    if merged and el is not None and k:
        base = foreach_leak_base(entries, ev.resources[res], k)
        if base is not None:
            el = merge_maps(base, el)
    return el


def rule_message(ev: Evaluation, rule, res: int) -> str:
    """RuleResponse.Message (validatePatterns, buildErrorMessage, buildAnyPatternErrorMessage:
    pkg/engine/validation.go:421-547): pass / fail from the status and failing path, skip / error
    from the device's error record rendered by ``kv_result_error_message``."""
    st = int(ev.status[rule.index, res])
    if st == ERROR and (rule.index, res) in ev.subst:  # ruleError("variable substitution failed", err)
        return ev.subst[(rule.index, res)]
    if st == SKIP and (rule.index, res) in ev.precond:  # "preconditions not met" (validation.go:183-184)
        return ev.precond[(rule.index, res)]
    if getattr(rule, "foreach", False):  # validateForEach (validation.go:204-283)
        if st == PASS:
            return "rule passed"
        if st in (FAIL, ERROR) and _pattern_entry(ev, rule, res):
            # the element's validatePatterns message: buildErrorMessage in the element's context
            # (validation.go:421-445,510-534)
            head = "validation failed in foreach rule for "
            path = ev.foreach_path.get((rule.index, res)) or ""
            tail = (f"failed at path {path}" if st == FAIL else
                    f"execution error: {ev.foreach_err.get((rule.index, res), '')}")
            if not rule.message:
                return head + f"validation error: rule {rule.name} {tail}"
            msg = _message(ev, rule, res, _foreach_element(ev, rule, res, merged=True))
            return head + f"validation error: {_with_dot(msg)} Rule {rule.name} {tail}"
        if st == FAIL and _any_entry(ev, rule, res):
            # the element's buildAnyPatternErrorMessage (validation.go:447-489,536-547): one part per
            # alternative, behind the rule's message as written (it is not substituted)
            parts = []
            for j, o in enumerate(ev.foreach_alts.get((rule.index, res), [])):
                if o is None:
                    continue
                _, path, text = o
                parts.append(f"Rule {rule.name}[{j}] failed at path {path}." if path else
                             f"Rule {rule.name}[{j}] failed: {text}.")
            es = " ".join(parts)
            head = "validation failed in foreach rule for "
            if not rule.message:
                return head + f"validation error: {es}"
            return head + f"validation error: {_with_dot(rule.message)} {es}"
        if st == FAIL:  # the element's validateDeny message, in the element's context
            head = "validation failed in foreach rule for "
            if not rule.message:
                return head + f"validation error: rule {rule.name} failed"
            try:
                return head + msgvars.substitute_message(rule.message, ev.resources[res],
                                                         _foreach_element(ev, rule, res, merged=True))
            except (msgvars.MessageVariableNotFound, msgvars.UnsupportedMessageVariable):
                return head + rule.message
        return ev.foreach.get((rule.index, res), "")  # ERROR, SKIP "rule skipped"
    if getattr(rule, "deny", False):  # validateDeny / getDenyMessage (validation.go:299-339)
        if st == PASS:
            return f"validation rule '{rule.name}' passed."
        if st == FAIL:
            if not rule.message:
                return f"validation error: rule {rule.name} failed"
            try:  # the substituted message as it is (no "validation error:" prefix) ...
                return _message(ev, rule, res)
            except msgvars.MessageVariableNotFound:  # ... or, when that errors, as written
                return rule.message
        if st == ERROR:  # ruleError("failed to substitute variables in deny conditions", err)
            return ev.deny.get((rule.index, res), "")
        return ""
    if rule.any_pattern:
        outs = ev.anypattern.get((rule.index, res), [])
        if st == PASS:
            j = next((j for j, (s, _) in enumerate(outs) if s == PASS), 0)
            return f"validation rule '{rule.name}' anyPattern[{j}] passed."
        errs = []
        for j, (s, detail) in enumerate(outs):
            if s == FAIL and detail:
                errs.append(f"Rule {rule.name}[{j}] failed at path {detail}.")
            elif s in (ERROR, SKIP) and detail is not None:
                errs.append(f"Rule {rule.name}[{j}] failed: {detail}.")
        es = " ".join(errs)
        if not rule.message:
            return f"validation error: {es}"
        return f"validation error: {_with_dot(rule.message)} {es}"
    if st == PASS:
        return f"validation rule '{rule.name}' passed."
    if st == FAIL:
        path = ev.paths.get((rule.index, res), "")
        if not rule.message:
            return f"validation error: rule {rule.name} failed at path {path}"
        msg = _message(ev, rule, res)
        return f"validation error: {_with_dot(msg)} Rule {rule.name} failed at path {path}"
    if st in (ERROR, SKIP) and (rule.index, res) in ev.errors:
        err = ev.errors[(rule.index, res)]
        if st == SKIP:  # ruleResponse(..., pe.Error(), RuleStatusSkip)
            return err
        if not rule.message:  # buildErrorMessage(err, "")
            return f"validation error: rule {rule.name} execution error: {err}"
        msg = _message(ev, rule, res)
        return f"validation error: {_with_dot(msg)} Rule {rule.name} execution error: {err}"
    if rule.const_message:
        return rule.const_message
    return ""


# ---------------------------------------------------------------- apply


@dataclass
class ResultCounts:
    """common.ResultCounts (pkg/kyverno/common/common.go:41-47)."""
    pass_: int = 0
    fail: int = 0
    warn: int = 0
    error: int = 0
    skip: int = 0
    routed: int = 0  # pairs of KV_ROUTE_CPU rules: evaluated by the reference engine, not here


def resource_path(res: dict) -> str:
    md = res.get("metadata") or {}
    return f"{md.get('namespace', '')}/{res.get('kind', '')}/{md.get('name', '')}"


def process_validate(ev: Evaluation, pi: int, res: int, rc: ResultCounts, policy_report: bool, out) -> dict:
    """ProcessValidateEngineResponse (common.go:703-766) for one (policy, resource): every policy
    rule found in the engine response is counted by its status, every other rule as skip; failures
    are printed with their index in the response. Returns the policyreport.Info result record."""
    policy = ev.policies[pi]
    rules = ev.policy_rules(pi)
    # the engine response holds the matched validate rules, in policy order (validation.go:78-106)
    resp = [r.index for r in rules if ev.status[r.index, res] != NOMATCH and r.route != ROUTE_NORESPONSE]
    printed = False
    violated = []
    for r in rules:
        if r.index in resp:
            i = resp.index(r.index)
            st = int(ev.status[r.index, res])
            if st == CPU:
                rc.routed += 1
                violated.append({"name": r.name, "status": "cpu", "message": ""})
                continue
            msg = rule_message(ev, r, res)
            if st == PASS:
                rc.pass_ += 1
            elif st == FAIL:
                rc.fail += 1
                if not policy_report:
                    if not printed:
                        out.write(f"\npolicy {policy['metadata']['name']} -> resource {resource_path(ev.resources[res])} "
                                  f"failed: \n")
                        printed = True
                    out.write(f"{i + 1}. {r.name}: {msg} \n")
            elif st == ERROR:
                rc.error += 1
            elif st == WARN:
                rc.warn += 1
            elif st == SKIP:
                rc.skip += 1
            violated.append({"name": r.name, "status": REPORT_STATUS[st], "message": msg})
        else:
            rc.skip += 1
            violated.append({"name": r.name, "status": "skip", "message": r.message})
    res_doc = ev.resources[res]
    md = res_doc.get("metadata") or {}
    return {"policy": policy["metadata"]["name"], "namespace": md.get("namespace", ""),
            "resource": {"kind": res_doc.get("kind", ""), "namespace": md.get("namespace", ""),
                         "apiVersion": res_doc.get("apiVersion", ""), "name": md.get("name", ""),
                         "uid": md.get("uid", "")},
            "rules": violated}


def policy_has_validate(policy: dict) -> bool:
    return any((r.get("validate") or None) is not None and r.get("validate") != {}
               for r in (policy.get("spec") or {}).get("rules") or [])


def apply(policy_paths: list[str], resource_paths: list[str], policy_report: bool = False, device: int = 0,
          out=sys.stdout, evaluation_fn=None, gpus: int = 1, deny: bool = False,
          foreach: bool = False, foreach_pattern: bool = False, foreach_entries: bool = False,
          foreach_anypattern: bool = False, foreach_patvars: bool = False) -> tuple[ResultCounts, list]:
    """applyCommandHelper (apply_command.go:147-310) for resource files. Returns counts and the
    policyreport infos. ``evaluation_fn(policies, resources) -> Evaluation`` replaces the device
    evaluation (tests of the host logic)."""
    policies = load_policies(policy_paths)
    resources = load_resources(resource_paths)
    return apply_docs(policies, resources, policy_report, device, out, evaluation_fn, gpus, deny, foreach, foreach_pattern,
                      foreach_entries, foreach_anypattern, foreach_patvars)


def apply_docs(policies: list[dict], resources: list[dict], policy_report: bool = False, device: int = 0,
               out=sys.stdout, evaluation_fn=None, gpus: int = 1, deny: bool = False,
          foreach: bool = False, foreach_pattern: bool = False, foreach_entries: bool = False,
          foreach_anypattern: bool = False, foreach_patvars: bool = False) -> tuple[ResultCounts, list]:
    mutated = autogen.mutate_policies(policies)
    if len(mutated) > 0 and len(resources) > 0:
        msg_p = "1 policy" if len(mutated) <= 1 else f"{len(policies)} policies"
        msg_r = "1 resource" if len(resources) <= 1 else f"{len(resources)} resources"
        out.write(f"\nApplying {msg_p} to {msg_r}... \n(Total number of result count may vary as the policy is "
                  f"mutated by Kyverno. To check the mutated policy please try with log level 5)\n")
    rc = ResultCounts()
    skipped = [p["metadata"]["name"] for p in mutated if has_unset_variables(p)]
    active = [p for p in mutated if not has_unset_variables(p)]
    infos = []
    if active and resources:
        ev = (evaluation_fn or (lambda p, r: evaluate(p, r, device=device, gpus=gpus, deny=deny, foreach=foreach,
                                                          foreach_pattern=foreach_pattern,
                                                          foreach_entries=foreach_entries,
                                                          foreach_anypattern=foreach_anypattern,
                                                          foreach_patvars=foreach_patvars)))(active, resources)
        for pi, pol in enumerate(active):
            if not policy_has_validate(pol):
                continue
            for res in range(len(resources)):
                infos.append(process_validate(ev, pi, res, rc, policy_report, out))
        for w in ev.warnings:
            print(f"warning: {w}", file=sys.stderr)
    if skipped:
        out.write(DIVIDER + "\n")
        out.write("Policies Skipped (as required variables are not provided by the user):\n")
        for i, n in enumerate(skipped):
            out.write(f"{i + 1}. {n}\n")
        out.write(DIVIDER + "\n")
    if policy_report:
        reports = build_policy_reports(infos)
        if reports or not resources:
            out.write(DIVIDER + "\nPOLICY REPORT:\n" + DIVIDER + "\n")
            out.write(json.dumps(reports, indent=2) + "\n")
        else:
            out.write(DIVIDER + "\nPOLICY REPORT: skip generating policy report (no validate policy found/resource "
                      "skipped)\n")
    else:
        out.write(f"\npass: {rc.pass_}, fail: {rc.fail}, warn: {rc.warn}, error: {rc.error}, skip: {rc.skip} \n")
    if rc.routed:
        out.write(f"(routed to the reference engine, not evaluated here: {rc.routed} rule results)\n")
    return rc, infos


def build_policy_reports(infos: list) -> list[dict]:
    """buildPolicyReports / buildPolicyResults / calculateSummary (pkg/kyverno/apply/report.go:23-179):
    one ClusterPolicyReport for cluster-scoped resources, one PolicyReport per namespace."""
    scopes: dict[str, list] = {}
    for info in infos:
        scope = f"policyreport-ns-{info['namespace']}" if info["namespace"] else "clusterpolicyreport"
        for r in info["rules"]:
            if r["status"] == "cpu":
                continue
            scopes.setdefault(scope, []).append({"policy": info["policy"], "rule": r["name"],
                                                 "message": r["message"], "result": r["status"],
                                                 "resources": [info["resource"]], "scored": True,
                                                 "source": "Kyverno"})
    reports = []
    for scope, results in scopes.items():
        summary = {k: sum(1 for x in results if x["result"] == k) for k in ("pass", "fail", "warn", "error", "skip")}
        rep = {"apiVersion": "wgpolicyk8s.io/v1alpha2",
               "kind": "ClusterPolicyReport" if scope == "clusterpolicyreport" else "PolicyReport",
               "metadata": {"name": scope}, "results": results, "summary": summary}
        if scope != "clusterpolicyreport":
            rep["metadata"]["namespace"] = scope[len("policyreport-ns-"):]
        reports.append(rep)
    return reports


# ---------------------------------------------------------------- test


def run_test(spec: dict, policies: list[dict], resources: list[dict], device: int = 0,
             evaluation_fn=None, deny: bool = False, foreach: bool = False) -> list[dict]:
    """`kyverno test` result matching (pkg/kyverno/test/test_command.go:347-494) for validate rules:
    the expected rule name falls back to autogen-<rule> / autogen-cronjob-<rule> when the policy's
    response does not hold it; a rule absent from the response is `skip`. Returns one row per
    expected result with the actual result ("cpu" for rules routed to the reference engine)."""
    mutated = autogen.mutate_policies(policies)
    ev = (evaluation_fn or (lambda p, r: evaluate(p, r, device=device, messages=False, deny=deny, foreach=foreach)))(mutated, resources)
    rows = []
    for t in spec["results"]:
        want = t.get("result") or t.get("status")
        actual = None
        for pi, pol in enumerate(mutated):
            if pol["metadata"]["name"] != t["policy"]:
                continue
            for res, rd in enumerate(resources):
                md = rd.get("metadata") or {}
                if md.get("name") != t["resource"]:
                    continue
                if t.get("kind") and rd.get("kind") != t["kind"]:
                    continue
                resp = {r.name: r for r in ev.policy_rules(pi)
                        if ev.status[r.index, res] != NOMATCH and r.route != ROUTE_NORESPONSE}
                for name in (t["rule"], "autogen-" + t["rule"], "autogen-cronjob-" + t["rule"]):
                    if name in resp:
                        st = int(ev.status[resp[name].index, res])
                        actual = "cpu" if st == CPU else REPORT_STATUS[st]
                        break
                else:
                    actual = "skip"
        rows.append({**t, "want": want, "actual": actual,
                     "ok": actual == want if actual not in (None, "cpu") else None})
    return rows


# ---------------------------------------------------------------- main


def main(argv: list[str] | None = None) -> int:
    ap = argparse.ArgumentParser(prog="kyverno", description="validate policies against resources on the GPU")
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("apply", help="applies policies on resources")
    a.add_argument("policies", nargs="+")
    a.add_argument("-r", "--resource", action="append", default=[], help="Path to resource files")
    a.add_argument("--policy-report", action="store_true", help="Generates policy report when passed")
    a.add_argument("--device", type=int, default=0, help="HIP device (first device with --gpus)")
    a.add_argument("--gpus", type=int, default=1, help="shard the resources over this many devices")
    a.add_argument("--device-deny", action="store_true",
                   help="evaluate validate.deny rules of the device forms on the GPU (KV_COMPILE_DENY)")
    a.add_argument("--device-foreach", action="store_true",
                   help="evaluate validate.foreach rules of the device forms on the GPU (KV_COMPILE_FOREACH)")
    a.add_argument("--device-foreach-pattern", action="store_true",
                   help="also evaluate validate.foreach entries that carry a pattern on the GPU "
                        "(KV_COMPILE_FOREACH_PATTERN; implies --device-foreach)")
    a.add_argument("--device-foreach-entries", action="store_true",
                   help="also evaluate validate.foreach rules of several entries on the GPU "
                        "(KV_COMPILE_FOREACH_ENTRIES; implies --device-foreach)")
    a.add_argument("--device-foreach-anypattern", action="store_true",
                   help="also evaluate validate.foreach entries that carry an anyPattern on the GPU "
                        "(KV_COMPILE_FOREACH_ANYPATTERN; implies --device-foreach-pattern and --device-foreach)")
    a.add_argument("--device-foreach-patvars", action="store_true",
                   help="also evaluate validate.foreach entries whose pattern holds {{element...}} / {{request.object...}} "
                        "variables on the GPU (KV_COMPILE_FOREACH_PATVARS; implies --device-foreach-pattern and "
                        "--device-foreach)")
    t = sub.add_parser("test", help="run tests from a directory holding test.yaml")
    t.add_argument("dir")
    t.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if args.cmd == "apply":
        try:
            rc, _ = apply(args.policies, args.resource, args.policy_report, args.device, gpus=args.gpus, deny=args.device_deny,
                          foreach=(args.device_foreach or args.device_foreach_pattern or args.device_foreach_entries
                                   or args.device_foreach_anypattern or args.device_foreach_patvars),
                          foreach_pattern=(args.device_foreach_pattern or args.device_foreach_anypattern
                                           or args.device_foreach_patvars),
                          foreach_entries=args.device_foreach_entries, foreach_anypattern=args.device_foreach_anypattern,
                          foreach_patvars=args.device_foreach_patvars)
        except msgvars.MessageVariableError as e:
            # the Go CLI dies in buildErrorMessage (msgRaw.(string), validation.go:519-524): a
            # panic, exit status 2
            print(f"panic: validate message substitution: {e}", file=sys.stderr)
            return 2
        return 1 if rc.fail > 0 or rc.error > 0 else 0
    import yaml

    failed = 0
    for f in _yaml_files(args.dir):
        if os.path.basename(f) != "test.yaml":
            continue
        d = os.path.dirname(f)
        spec = yaml.safe_load(open(f))
        pols = load_policies([os.path.join(d, p) for p in spec.get("policies", [])])
        ress = load_resources([os.path.join(d, r) for r in spec.get("resources", [])])
        rows = run_test(spec, pols, ress, args.device)
        print(f"\nExecuting {spec.get('name', d)}...")
        for i, r in enumerate(rows):
            verdict = {True: "Pass", False: "Fail", None: "routed to reference engine"}[r["ok"]]
            print(f"{i + 1:3d} {r['policy']:30s} {r['rule']:30s} {r['resource']:35s} {verdict}")
            failed += r["ok"] is False
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
