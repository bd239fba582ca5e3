"""Shared data of the anyPattern-entry foreach tests (test_foreach_anypattern_cpu.py,
test_gpu_foreach_anypattern.py): the crafted rule set over foreach_pattern_data.crafted_resources
and the expected side.

The expectation is the decomposition of foreach_pattern_data.py / foreach_chain_model.py with the
entry's `anyPattern` in the last step (pkg/engine/validation.go:175-202, 447-489, 536-547): per
element the alternatives are tried in order with `oracle.match_pattern(element, alternative)` in
its float mode (res_mode 0); the first that returns no error makes the element PASS and ends the
loop; every error, one with `skip` set included, is collected as "Rule <name>[<idx>] failed at path
<path>." (a path) or "Rule <name>[<idx>] failed: <text>." (none); no alternative passing is FAIL,
never SKIP or ERROR. An element is CPU when an alternative up to and including the first that
passes meets an int-typed number under a pattern string that compares its text form
(foreach_pattern_data.meets_int). The message is the rule's text as written.

The device also makes an element CPU when an alternative's error record does not fit its 8-byte
form (kvwalk.h: an error behind a level-3 loop or a level-0 loop of 1024 iterations or more). This
model has no notion of that, and the parity tests hold because the crafted data produces no such
record: its only loops are over `ports` of 0 to 3 entries, one level deep.
"""
from __future__ import annotations

import json

import numpy as np

import cond_model
import foreach_chain_model
import foreach_data as fd
import foreach_model
import foreach_pattern_data as fpd
import precond_data as pd

PASS, FAIL, WARN, ERROR, SKIP, NOMATCH, CPU = range(7)
STATUS = fd.STATUS
POD = pd.POD
LIST, INIT = fd.LIST, fd.INIT
HEAD = foreach_model.HEAD
# rules that stay on the CPU route with every flag on
CPU_RULES = ("any-and-pattern", "any-and-deny", "any-and-context", "any-not-a-list", "any-empty", "any-non-map",
             "any-nine", "any-variable", "any-metadata", "any-reference-absolute", "any-reference-climbing",
             "any-reference-inside")
NAMES8 = [{"name": f"c{j}"} for j in range(1, 9)]


def _rule(name, alts, message="", pre=None, epre=None, lst=LIST):
    entry = {"list": lst, "anyPattern": alts}
    if epre is not None:
        entry["preconditions"] = epre
    r = {"name": name, "match": POD, "validate": {"message": message, "foreach": [entry]}}
    if pre is not None:
        r["preconditions"] = pre
    return r


def _raw(name, entry):
    return {"name": name, "match": POD, "validate": {"message": "m", "foreach": [entry]}}


def crafted_policy():
    rules = [
        # the message is not substituted: {{element.name}} stays as written (no trailing dot)
        _rule("latest-or-c0", [{"image": "!*:latest"}, {"name": "c0"}], "image of {{element.name}} is tagged latest"),
        _rule("three", [{"image": "reg0.io/*"}, {"name": "c1 | c2"}, {"tier": "ok"}], "one of three."),
        # a condition anchor: its mismatch is a PatternError with `skip` set and no path; a container
        # without `tier` is an error without a path (the anchor key is missing)
        _rule("cond-anchor", [{"(tier)": "ok", "image": "reg0.io/*"}, {"name": "c0"}]),
        _rule("global-anchor", [{"<(image)": "reg1.io/*", "port": 80}, {"port": 8080}], "global"),
        # alternative 0 loops over `ports` (the lanes of a wave hold 0-3 entries), alternative 1
        # fails outside any loop: the wave's loop counters must be cleared in between
        _rule("ports-then-name", [{"=(ports)": [{"containerPort": "<1024"}], "name": "c1 | c3"}, {"name": "c0"}], "ports"),
        _rule("eight", NAMES8),
        _rule("gated", [{"image": "reg0.io/*"}, {"image": "reg1.io/*"}],
              epre={"all": [{"key": "{{element.name}}", "operator": "NotEquals", "value": "c0"}]}),
        _rule("behind-preconditions", [{"image": "!*:latest"}, {"name": "c0"}],
              pre={"all": [{"key": fd.APP, "operator": "NotEquals", "value": "db"}]}),
        _rule("init-containers", [{"image": "reg0.io/*"}, {"image": "reg1.io/*"}], lst=INIT),
        _rule("first-container", [{"name": "c1"}, {"port": 8080}], lst=LIST + "[0]"),
        _rule("shared", [{"image": "!*:latest"}, {"name": "c0"}], "shared"),
        # several entries: a deny entry, then an anyPattern entry
        {"name": "deny-then-any", "match": POD, "validate": {"message": "chain", "foreach": [
            {"list": INIT, "deny": {"conditions": {"all": [
                {"key": "{{element.image}}", "operator": "Equals", "value": "busybox"}]}}},
            {"list": LIST, "anyPattern": [{"image": "reg0.io/*"}, {"name": "c1 | c2"}, {"tier": "ok"}]}]}},
        # outside the scope at compile time
        _raw("any-and-pattern", {"list": LIST, "anyPattern": [{"name": "c*"}], "pattern": {"name": "c*"}}),
        _raw("any-and-deny", {"list": LIST, "anyPattern": [{"name": "c*"}], "deny": {"conditions": {"all": [
            {"key": "{{element.name}}", "operator": "Equals", "value": "x"}]}}}),
        _raw("any-and-context", {"list": LIST, "anyPattern": [{"name": "c*"}],
                                 "context": [{"name": "x", "configMap": {"name": "a", "namespace": "b"}}]}),
        _raw("any-not-a-list", {"list": LIST, "anyPattern": {"name": "c*"}}),
        _raw("any-empty", {"list": LIST, "anyPattern": []}),
        _raw("any-non-map", {"list": LIST, "anyPattern": [{"name": "c*"}, "c*"]}),
        _raw("any-nine", {"list": LIST, "anyPattern": NAMES8 + [{"name": "c9"}]}),
        _raw("any-variable", {"list": LIST, "anyPattern": [{"name": "c0"}, {"name": "{{element.name}}"}]}),
        _raw("any-metadata", {"list": LIST, "anyPattern": [{"name": "c0"}, {"(metadata)": {"name": "x"}}]}),
        # $() references: the reference substitutes the anyPattern list as one document, alternative k
        # at /k/..., so an absolute reference or one that climbs above its alternative fails to
        # resolve and every element is an ERROR; the alternatives are compiled one by one on the
        # device, so an entry with a reference anywhere stays routed
        _raw("any-reference-absolute", {"list": LIST, "anyPattern": [{"name": "$(/image)", "image": "x"}]}),
        _raw("any-reference-climbing", {"list": LIST, "anyPattern": [{"name": "c0"}, {"name": "$(../../../image)", "image": "x"}]}),
        _raw("any-reference-inside", {"list": LIST, "anyPattern": [{"name": "$(./../image)", "image": "x"}]}),
    ]
    return pd._policy("crafted-foreach-anypattern", rules)


def int_policy():
    """Outside the CPU cap. port-glob-first: alternative 0 compares the number's text form, so every
    element with an int port is CPU. name-first: alternative 0 passes on c0 before the guarded
    alternative is reached (the guard does not count for it); c1.. reach it."""
    return pd._policy("foreach-anypattern-int", [_rule("port-glob-first", [{"port": "?0"}, {"name": "?*"}]),
                                                  _rule("name-first", [{"name": "c0"}, {"port": "?0"}])])


def crafted_resources(n, float_ports=False):
    return fpd.crafted_resources(n, float_ports)


def on_device(rule) -> bool:
    return fd.is_foreach(rule) and rule["name"] not in CPU_RULES


def n_alternatives(rule) -> int:
    """The alternative count of a device rule of one anyPattern entry, else 0."""
    fe = rule["validate"]["foreach"]
    return len(fe[0]["anyPattern"]) if on_device(rule) and len(fe) == 1 and "anyPattern" in fe[0] else 0


class Model(foreach_chain_model.Model):
    """foreach_chain_model.Model with anyPattern entries."""

    def any_element(self, entry, resource, raw, seen):
        """validate() on one element of an anyPattern entry: (code, detail). detail: ("pass", the
        alternative that passed) or ("fail", the oracle's error per alternative)."""
        pre = entry.get("preconditions")
        if pre is not None:
            v = self.lenient.preconditions(pre, (resource, seen))
            if v == cond_model.UNKNOWN:
                return "cpu", None
            if v is False:
                return "skip", None
        errs = []
        for a, alt in enumerate(entry["anyPattern"]):
            if fpd.meets_int(self.orc, alt, raw):
                return "cpu", None
            key = (json.dumps(raw, sort_keys=True), json.dumps(alt, sort_keys=True))
            got = self._memo.get(key)
            if got is None:
                got = self._memo[key] = self.orc.match_pattern(json.dumps(raw), json.dumps(alt), res_mode=0)
            assert "panic" not in got, got
            if not got["set"]:
                return "pass", ("pass", a)
            errs.append(got)
        return "fail", ("fail", errs)

    @staticmethod
    def any_message(rule, errs):
        """buildAnyPatternErrorMessage (validation.go:536-547) over the collected errors."""
        name, msg = rule["name"], rule["validate"].get("message", "")
        parts = " ".join(f"Rule {name}[{a}] failed at path {e['path']}." if e["path"] else f"Rule {name}[{a}] failed: {e['msg']}."
                         for a, e in enumerate(errs))
        if not msg:
            return f"validation error: {parts}"
        return f"validation error: {msg if msg.endswith('.') else msg + '.'} {parts}"

    def chain(self, rule, resource, codes=None):
        """foreach_chain_model.Model.chain with the anyPattern branch; `codes`: a list that receives
        (code, detail) of every element the walk evaluated."""
        base = None
        applied = 0
        for k, entry in enumerate(rule["validate"]["foreach"]):
            state, elems = self.elements(entry["list"], resource)
            if state == "cpu":
                return "cpu", k, None, None, None
            if state == "empty":
                continue
            for i, raw in enumerate(elems):
                seen = raw if base is None else foreach_chain_model.merge(base, raw)
                detail = None
                if "anyPattern" in entry:
                    c, detail = self.any_element(entry, resource, raw, seen)
                    msgs = [HEAD + self.any_message(rule, detail[1])] if c == "fail" else None
                elif "pattern" in entry:
                    c, detail = self.pattern_element(rule, entry, resource, raw, seen)
                    msgs = [HEAD + self.pattern_message(rule, resource, seen, detail)] if c in ("fail", "error") else None
                else:
                    c, msgs = self.element(rule, entry, resource, seen)
                if codes is not None:
                    codes.append((c, detail))
                if c == "skip":
                    continue
                if c == "pass":
                    applied += 1
                    continue
                return c, k, i, msgs, detail
            if elems and self.leak:
                base = elems[-1] if base is None else foreach_chain_model.merge(base, elems[-1])
        return (("pass", None, None, [foreach_model.PASSED], None) if applied else
                ("skip", None, None, [foreach_model.SKIPPED], None))

    def all_codes(self, rule, resource):
        """(code, detail) of every element of a rule of one entry (no early exit)."""
        entry = rule["validate"]["foreach"][0]
        state, elems = self.elements(entry["list"], resource)
        return [] if state != "ok" else [self.any_element(entry, resource, e, e) for e in elems]


def alt_status(err) -> int:
    """The status of one alternative that did not pass, as the walk's epilogue names it."""
    return SKIP if err["skip"] else FAIL if err["path"] else ERROR


class Expected(fpd.Expected):
    """The decomposition for one policy over resources: statuses and, per FAIL pair an anyPattern
    entry decided, the deciding entry and element and per alternative (status, path | None, text);
    the RuleResponse message of every decided pair."""

    def __init__(self, orc, policy, resources):
        self.orc = orc
        self.lenient = cond_model.Model(orc)
        self.model = Model(orc)
        ost, _ = orc.validate_batch(json.dumps([fd.match_policy(policy)]), json.dumps(resources), nthreads=8)
        ost = ost.copy()
        ost[ost == 7] = CPU
        rules = policy["spec"]["rules"]
        self.rules, self.resources = rules, resources
        self.status = ost.copy()
        self.elem, self.entry, self.alts, self.messages, self.codes = {}, {}, {}, {}, {}
        for ri, rule in enumerate(rules):
            if not fd.is_foreach(rule):
                continue
            for k, res in enumerate(resources):
                if ost[ri, k] == NOMATCH:
                    continue
                if not on_device(rule):
                    self.status[ri, k] = CPU
                    continue
                assert ost[ri, k] == PASS, (rule["name"], k, ost[ri, k])
                if "preconditions" in rule:
                    p = self.lenient.preconditions(rule["preconditions"], res)
                    if p == cond_model.UNKNOWN:
                        self.status[ri, k] = CPU
                        continue
                    if p is False:
                        self.status[ri, k] = SKIP
                        self.messages[(ri, k)] = fd.NOT_MET
                        continue
                if n_alternatives(rule):
                    self.codes[(ri, k)] = self.model.all_codes(rule, res)
                v, ent, el, msgs, detail = self.model.chain(rule, res)
                self.status[ri, k] = STATUS[v]
                if v in ("fail", "error"):
                    self.elem[(ri, k)] = el
                    self.entry[(ri, k)] = ent
                    if detail is not None and detail[0] == "fail":
                        self.alts[(ri, k)] = [(alt_status(e), e["path"] or None, e["msg"]) for e in detail[1]]
                if v != "cpu" and msgs and len(msgs) == 1:
                    self.messages[(ri, k)] = msgs[0]

    def check_honest(self, full: bool):
        """Conditions on the inputs, from the model alone: at most 10 % of the matched device pairs
        are CPU; at the full size PASS is decided by alternative 0 and by a later one, FAIL by first,
        middle and last elements, both part forms occur, and some resource's elements mix "passes at
        alternative 0" and "needs every alternative" (parked and running lanes share a wave)."""
        pairs = self.device_pairs([ri for ri, r in enumerate(self.rules) if on_device(r)])
        if len(pairs) >= 100:
            assert (pairs == CPU).sum() * 10 <= len(pairs), ((pairs == CPU).sum(), len(pairs))
        if not full:
            return
        passed_at, where, forms, mixed = set(), set(), set(), False
        for (ri, k), cs in self.codes.items():
            n_alt = n_alternatives(self.rules[ri])
            at0 = every = False
            for c, d in cs:
                if c == "pass":
                    passed_at.add(min(d[1], 1))
                    at0 |= d[1] == 0
                    every |= d[1] == n_alt - 1 and n_alt > 1
                every |= c == "fail"
            mixed |= at0 and every and len(cs) >= 64
            if self.status[ri, k] == FAIL and (ri, k) in self.alts:
                e = self.elem[(ri, k)]
                where.add("first" if e == 0 else "last" if e == len(cs) - 1 else "middle")
                forms |= {"path" if p else "text" for _, p, _ in self.alts[(ri, k)]}
        assert passed_at == {0, 1}, passed_at
        assert where >= {"first", "middle", "last"}, where
        assert forms == {"path", "text"}, forms
        assert mixed
