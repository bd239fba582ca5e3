"""Shared data of the tests of `{{element...}}` variables in foreach pattern entries
(test_foreach_patvars_cpu.py, test_gpu_foreach_patvars.py): the crafted rule set, its resources and
the expected side.

The expectation is the decomposition of foreach_anypattern_data.py / foreach_chain_model.py with one
step added in front of the element's pattern match (pkg/engine/validation.go:175-202, 549-571
substitutePatterns): after the entry preconditions the whole `pattern` (the whole `anyPattern`
list) is substituted in the element's context with the strict resolver. The oracle does it: every
`{{element` of the pattern is rewritten to `{{request.object.element` and
`oracle.substitute_vars(pattern, dict(resource, element=<element or leak overlay>))` gives
 * {"doc"}: the substituted pattern, matched with `oracle.match_pattern(element, doc, res_mode=0)`;
 * {"error"}: the element is ERROR, "variable substitution failed: <error>";
 * {"scope": False}: the element is CPU.
An element is CPU too where a map or an array replaced a leaf (the device has no structural
substitution), and where the int-typing rule of foreach_pattern_data.meets_int holds on the
*substituted* pattern (a substituted glob over an int-typed number).
"""
from __future__ import annotations

import copy
import json
import re

import numpy as np

import cond_model
import foreach_anypattern_data as fad
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
SUBST = "variable substitution failed: "
# rules that stay on the CPU route with every flag on
CPU_RULES = ("var-in-key", "whole-element", "at-variable", "function", "nested", "escape", "reference-brings-variable",
             "metadata-key", "any-var-in-key")
ALL = dict(foreach=True, foreach_pattern=True, foreach_entries=True, foreach_anypattern=True, foreach_patvars=True)
_ELEMENT = re.compile(r"\{\{(\s*)element")
_ROOT = re.compile(r"request\.object\.([A-Za-z_][A-Za-z0-9_]*)")


def _rule(name, pattern, message="", pre=None, epre=None, lst=LIST):
    return fpd._rule(name, pattern, message, pre, epre, lst)


def crafted_policy():
    never = {"conditions": {"all": [{"key": "{{element.image}}", "operator": "Equals", "value": "never"}]}}
    rules = [
        # the reference's own form (Test_foreach_element_validation), with the spaces
        _rule("name-is-alias", {"name": "{{ element.alias }}"}, "alias of {{element.name}}"),
        # a condition anchor in front: an element without `tier` is an ERROR of the walk (no path),
        # one without `alias` an ERROR of the substitution, which comes first
        _rule("tier-alias", {"(tier)": "ok", "name": "{{element.alias}}"}, "tier ok needs its alias"),
        # request.object variables; `labels` is missing on some resources
        _rule("owner-is-app", {"=(owner)": "{{request.object.metadata.labels.app}}"}),
        # several variables in one string, numbers spliced as text, around a glob
        _rule("image-parts", {"image": "reg{{element.regno}}.io/app{{ element.appno }}:*"}, "image parts"),
        # a whole-string number keeps its type: float64 against the element's number
        _rule("port-copy", {"port": "{{element.portcopy}}"}),
        # a variable inside a list of maps: the lanes of a wave loop over 0-3 ports
        _rule("ports-are-pc", {"=(ports)": [{"name": "p*", "containerPort": "{{element.pc}}"}]}, "ports"),
        # two strings, both orders of outcomes occur: `a-alias` comes before `name` in traversal order
        _rule("two-strings", {"name": "{{element.alias}}", "=(a-alias)": "{{element.second}}"}),
        _rule("gated", {"name": "{{element.alias}}"},
              epre={"all": [{"key": "{{element.name}}", "operator": "NotEquals", "value": "c0"}]}),
        _rule("behind-preconditions", {"name": "{{ element.alias }}"},
              pre={"all": [{"key": fd.APP, "operator": "NotEquals", "value": "db"}]}),
        _rule("init-containers", {"image": "reg?.io/*", "name": "{{element.name}}"}, lst=INIT),
        _rule("shared", {"name": "{{ element.alias }}"}, "shared"),
        # a pattern without variables next to them: its set runs what it ran before
        _rule("no-latest", {"image": "!*:latest"}, "image of {{element.name}} is tagged latest"),
        # anyPattern: alternative 0 has no variable and matches c0; the string of alternative 1 is
        # substituted before alternative 0 is tried
        {"name": "any-c0-or-alias", "match": POD, "validate": {"message": "any", "foreach": [
            {"list": LIST, "anyPattern": [{"name": "c0"}, {"name": "{{element.alias}}"}]}]}},
        {"name": "any-two-vars", "match": POD, "validate": {"message": "any two.", "foreach": [
            {"list": LIST, "anyPattern": [{"image": "reg{{element.regno}}.io/nope*"}, {"port": "{{element.portcopy}}"}]}]}},
        # several entries: the second entry's {{element.mark}} is a key of initContainers' last
        # element only: it resolves through the leak, and not at all without initContainers
        {"name": "deny-then-leaked", "match": POD, "validate": {"message": "chain", "foreach": [
            {"list": INIT, "deny": copy.deepcopy(never)},
            {"list": LIST, "pattern": {"name": "{{element.mark}}*"}}]}},
        # outside the scope at compile time
        _rule("var-in-key", {"{{element.name}}": "x"}),
        _rule("whole-element", {"name": "{{element}}"}),
        _rule("at-variable", {"name": "{{@}}"}),
        _rule("function", {"name": "{{ to_upper(element.name) }}"}),
        _rule("nested", {"name": "{{ element.{{request.object.metadata.name}} }}"}),
        _rule("escape", {"name": "{{element.alias}}", "image": "\\{{element.image}}"}),
        _rule("reference-brings-variable", {"image": "{{element.alias}}", "name": "$(./../image)"}),
        _rule("metadata-key", {"metadata": {"name": "{{element.name}}"}}),
        {"name": "any-var-in-key", "match": POD, "validate": {"message": "m", "foreach": [
            {"list": LIST, "anyPattern": [{"name": "c0"}, {"{{element.name}}": "x"}]}]}},
    ]
    return pd._policy("crafted-foreach-patvars", rules)


def int_policy():
    """Outside the CPU cap: a substituted glob ("?0") over the port. On int ports every element with
    the glob is CPU; on 0.5-style ports the glob is evaluated on the float's text form."""
    return pd._policy("foreach-patvars-int", [_rule("port-glob", {"port": "{{element.portglob}}"}),
                                              _rule("name-set", {"name": "{{element.name}}"})])


def crafted_resources(n, float_ports=False):
    """foreach_pattern_data.crafted_resources with the fields the variables read, on container j of
    resource i: `alias` (the name; another name on some, missing on some, a map on a few), `regno` /
    `appno` (the numbers inside `image`; wrong on some), `portcopy` (the port, wrong on some), `pc`
    (80), `owner` (on some: the app label or "nobody"), `second` ("s"; missing on some, a list on
    some) with `a-alias` on some ("s" or "t"), `portglob` ("?0"), and `mark` on the last initContainer."""
    out = fpd.crafted_resources(n, float_ports)
    for i, res in enumerate(out):
        cs = res["spec"].get("containers")
        for j, c in enumerate(cs if isinstance(cs, list) else [cs]):
            if not isinstance(c, dict):
                continue
            if (i * 5 + j) % 29 == 7 or (i % 16 == 2 and j == 63) or (i == 1 and j == 69):
                pass  # no alias: a substitution error
            elif i % 31 == 12 and j == 1:
                c["alias"] = {"a": 1}
            elif (i + 3 * j) % 41 == 0:
                c["alias"] = "x" + c["name"]
            else:
                c["alias"] = c["name"]
            c["regno"] = (i + j) % 3 if (i + 2 * j) % 37 else 7
            c["appno"] = j
            c["portcopy"] = c["port"] if (i * 3 + j) % 23 else 81
            c["pc"] = 80
            c["portglob"] = "?0"
            if (i + j) % 6 == 0:
                c["owner"] = res["metadata"].get("labels", {}).get("app", "web") if (i + j) % 12 else "nobody"
            if (i + j) % 9 in (1, 4):
                c["a-alias"] = "s" if (i + j) % 9 == 1 else "t"
            if (i + j) % 27 == 1 and i % 5 == 0:
                c["second"] = ["s"]
            elif (i + j) % 27 != 10:
                c["second"] = "s"
        init = res["spec"].get("initContainers")
        if init:
            init[-1]["mark"] = "c0"
    return out


def on_device(rule) -> bool:
    return fd.is_foreach(rule) and rule["name"] not in CPU_RULES


def has_variable(x) -> bool:
    if isinstance(x, str):
        return "{{" in x
    if isinstance(x, dict):
        return any(has_variable(v) for v in x.values())
    if isinstance(x, list):
        return any(has_variable(v) for v in x)
    return False


def rule_has_variables(rule) -> bool:
    return on_device(rule) and any(has_variable(e.get("pattern")) or has_variable(e.get("anyPattern"))
                                   for e in rule["validate"]["foreach"])


def _structural(pattern, doc) -> bool:
    """A variable string of `pattern` became a map or an array in `doc`."""
    if isinstance(pattern, str):
        return isinstance(doc, (dict, list))
    if isinstance(pattern, dict):
        return any(_structural(v, doc[k]) for k, v in pattern.items())
    if isinstance(pattern, list):
        return any(_structural(p, d) for p, d in zip(pattern, doc))
    return False


class Model(fad.Model):
    """foreach_anypattern_data.Model with substitutePatterns in front of the match."""

    def __init__(self, orc):
        super().__init__(orc)
        self._subst = {}

    def substitute(self, pattern, resource, seen):
        """("doc", substituted pattern) | ("error", text) | ("cpu", None), in the context of the
        element as the variables see it."""
        if not has_variable(pattern):
            return "doc", pattern
        raw = json.dumps(pattern)
        text = _ELEMENT.sub(r"{{\1request.object.element", raw)
        # (a field chain reads along its path only: the context keeps the top-level keys of the
        # resource that a request.object variable of the pattern names, which keeps a Pod of 300
        # containers out of every call)
        ctx = {k: resource[k] for k in set(_ROOT.findall(raw)) if k in resource}
        ctx["element"] = seen
        key = (text, json.dumps(ctx, sort_keys=True))
        got = self._subst.get(key)
        if got is None:
            got = self._subst[key] = self.orc.substitute_vars(json.loads(text), ctx)
        if "error" in got:
            return "error", got["error"]
        if "doc" not in got:
            return "cpu", None
        if _structural(pattern, got["doc"]):
            return "cpu", None
        return "doc", got["doc"]

    def _gate(self, entry, resource, seen):
        pre = entry.get("preconditions")
        if pre is not None:
            v = self.lenient.preconditions(pre, (resource, seen))
            if v == cond_model.UNKNOWN:
                return "cpu"
            if v is False:
                return "skip"
        return None

    def _match(self, raw, pat):
        key = (json.dumps(raw, sort_keys=True), json.dumps(pat, sort_keys=True))
        got = self._memo.get(key)
        if got is None:
            got = self._memo[key] = self.orc.match_pattern(json.dumps(raw), json.dumps(pat), res_mode=0)
        assert "panic" not in got, got
        return got

    def pattern_element(self, rule, entry, resource, raw, seen):
        g = self._gate(entry, resource, seen)
        if g:
            return g, None
        kind, pat = self.substitute(entry["pattern"], resource, seen)
        if kind == "error":
            return "error", {"subst": pat, "path": "", "msg": None}
        if kind == "cpu" or fpd.meets_int(self.orc, pat, raw):
            return "cpu", None
        got = self._match(raw, pat)
        if not got["set"]:
            return "pass", None
        if got["skip"]:
            return "skip", None
        return ("error" if got["path"] == "" else "fail"), got

    def pattern_message(self, rule, resource, seen, detail):
        if detail.get("subst") is not None:
            return SUBST + detail["subst"]
        return super().pattern_message(rule, resource, seen, detail)

    def any_element(self, entry, resource, raw, seen):
        g = self._gate(entry, resource, seen)
        if g:
            return g, None
        kind, alts = self.substitute(entry["anyPattern"], resource, seen)
        if kind == "error":
            return "error", ("subst", alts)
        if kind == "cpu":
            return "cpu", None
        errs = []
        for a, alt in enumerate(alts):
            if fpd.meets_int(self.orc, alt, raw):
                return "cpu", None
            got = self._match(raw, alt)
            if not got["set"]:
                return "pass", ("pass", a)
            errs.append(got)
        return "fail", ("fail", errs)

    def chain(self, rule, resource, codes=None):
        """foreach_anypattern_data.Model.chain with the substitution error of an anyPattern entry."""
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
                    msgs = ([HEAD + self.any_message(rule, detail[1])] if c == "fail" else
                            [HEAD + SUBST + detail[1]] if c == "error" else None)
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
        if state != "ok":
            return []
        if "anyPattern" in entry:
            return [self.any_element(entry, resource, e, e) for e in elems]
        return [self.pattern_element(rule, entry, resource, e, e) for e in elems]


def is_subst(detail) -> bool:
    """The detail of an ERROR element names a substitution error (a pattern entry's or an any entry's)."""
    return (isinstance(detail, dict) and detail.get("subst") is not None) or \
        (isinstance(detail, tuple) and detail[0] == "subst")


class Expected(fpd.Expected):
    """The decomposition for one policy over resources: statuses; per FAIL / ERROR pair the deciding
    entry and element; `path` / `err` (the failing path, the pattern error's text) where a pattern
    entry's walk decided; `subst` (the whole message) where the substitution decided; `alts` as
    foreach_anypattern_data.Expected; the RuleResponse message of every decided pair; `codes`:
    every element's (code, detail) for the rules of one entry."""

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
        self.path, self.err, self.subst = {}, {}, {}
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
                if len(rule["validate"]["foreach"]) == 1:
                    self.codes[(ri, k)] = self.model.all_codes(rule, res)
                v, ent, el, msgs, detail = self.model.chain(rule, res)
                self.status[ri, k] = STATUS[v]
                if v in ("fail", "error"):
                    self.elem[(ri, k)] = el
                    self.entry[(ri, k)] = ent
                    if v == "error" and is_subst(detail):
                        self.subst[(ri, k)] = msgs[0]
                    elif isinstance(detail, tuple) and detail[0] == "fail":
                        self.alts[(ri, k)] = [(fad.alt_status(e), e["path"] or None, e["msg"]) for e in detail[1]]
                    elif isinstance(detail, dict):
                        self.err[(ri, k)] = detail["msg"]
                        if v == "fail":
                            self.path[(ri, k)] = detail["path"]
                if v != "cpu" and msgs and len(msgs) == 1:
                    self.messages[(ri, k)] = msgs[0]

    def check_honest(self, full: bool = False):
        """Conditions on the inputs, from the model alone: at most 10 % of the matched device pairs
        are CPU (sets of 100 pairs or more); at sizes from 63 on one rule yields PASS, FAIL, ERROR, SKIP
        and CPU, ERROR pairs come from the substitution and from the pattern walk, a substitution ERROR
        is decided by a first, a middle and a last element, and in an anyPattern rule a failing
        string of alternative 1 makes an element ERROR that alternative 0 would match."""
        names = [r["name"] for r in self.rules]
        pairs = self.device_pairs([ri for ri, r in enumerate(self.rules) if on_device(r)])
        if len(pairs) >= 100:
            assert (pairs == CPU).sum() * 10 <= len(pairs), ((pairs == CPU).sum(), len(pairs))
        if len(self.resources) < 63:
            return
        one = self.device_pairs([names.index("name-is-alias")])
        for s in (PASS, FAIL, ERROR, SKIP, CPU):
            assert (one == s).any(), s
        errors = [key for key in self.elem if self.status[key] == ERROR]
        assert any(key in self.subst for key in errors) and any(key in self.err for key in errors)
        where = set()
        for (ri, k) in self.subst:
            cs = self.codes.get((ri, k))
            if cs is None or len(cs) < 3:
                continue
            e = self.elem[(ri, k)]
            where.add("first" if e == 0 else "last" if e == len(cs) - 1 else "middle")
        assert where >= {"first", "middle", "last"}, where
        ai = names.index("any-c0-or-alias")
        alt0 = self.rules[ai]["validate"]["foreach"][0]["anyPattern"][0]
        assert not has_variable(alt0)
        hit = False
        for (ri, k), cs in self.codes.items():
            if ri != ai:
                continue
            _, elems = self.model.elements(LIST, self.resources[k])
            for (c, d), raw in zip(cs, elems or []):
                if c == "error" and is_subst(d) and not self.model._match(raw, alt0)["set"]:
                    hit = True
        assert hit
