"""Shared data of the pattern-entry foreach tests (test_foreach_pattern_cpu.py,
test_gpu_foreach_pattern.py): the crafted rule set, its resources and the expected side.

The expectation is the decomposition of foreach_data.py with the entry's `pattern` in the last
step: the oracle for match / exclude, cond_model.py for the rule's and the entry's preconditions,
foreach_model.py for the list states and the reduction, and per element
`oracle.match_pattern(element, pattern)` in its float mode (res_mode 0: every number of the
element float64, which is how the reference types an element that comes out of the JSON context):
no error PASS, `skip` SKIP (ignored), an empty path ERROR, else FAIL with the element-relative path.
An element is CPU where the device cannot show parity: a number the store types int64 (a JSON
literal that parses as one) meets a string pattern that compares its text form.
"""
from __future__ import annotations

import json
import re

import numpy as np

import cond_model
import foreach_data as fd
import foreach_model
import precond_data as pd

PASS, FAIL, WARN, ERROR, SKIP, NOMATCH, CPU = range(7)
STATUS = fd.STATUS
POD = pd.POD
LIST, INIT = fd.LIST, fd.INIT
HEAD = foreach_model.HEAD
# rules that stay on the CPU route with both flags on
CPU_RULES = ("entry-any-pattern", "pattern-variable", "pattern-metadata", "pattern-and-deny", "two-entries",
             "pattern-not-a-map")


def _rule(name, pattern, message="", pre=None, epre=None, lst=LIST):
    entry = {"list": lst, "pattern": pattern}
    if epre is not None:
        entry["preconditions"] = epre
    r = {"name": name, "match": POD, "validate": {"message": message, "foreach": [entry]}}
    if pre is not None:
        r["preconditions"] = pre
    return r


def crafted_policy():
    rules = [
        _rule("no-latest", {"image": "!*:latest"}, "image of {{element.name}} is tagged latest"),
        _rule("tier-if-set", {"=(tier)": "ok"}),
        # a condition anchor: elements without tier "ok" are SKIP, the others checked; a container
        # without `tier` is an ERROR (the anchor key is missing)
        _rule("tier-image", {"(tier)": "ok", "image": "reg0.io/*"}, "tier ok needs reg0"),
        _rule("global-image", {"<(image)": "reg1.io/*", "port": 80}),
        _rule("high-port", {"port": ">1000"}, "port of {{element.name}} too low"),
        _rule("no-tier", {"X(tier)": "null"}),
        _rule("cpu-limit", {"resources": {"limits": {"cpu": "?*"}}}),
        _rule("low-container-ports", {"=(ports)": [{"containerPort": "<1024"}]}, "privileged ports only"),
        _rule("one-tls-port", {"^(ports)": [{"containerPort": 8443}]}),
        _rule("p1-is-80", {"=(ports)": [{"(name)": "p1", "containerPort": 80}]}),
        _rule("has-tier", {"tier": "*"}),
        _rule("gated", {"image": "reg0.io/*"},
              epre={"all": [{"key": "{{element.name}}", "operator": "NotEquals", "value": "c0"}]}),
        _rule("behind-preconditions", {"image": "!*:latest"},
              pre={"all": [{"key": fd.APP, "operator": "NotEquals", "value": "db"}]}),
        _rule("init-containers", {"image": "reg?.io/*"}, lst=INIT),
        _rule("first-container", {"name": "c0", "port": 8080}, lst=LIST + "[0]"),
        _rule("shared", {"image": "!*:latest"}, "shared"),
        # outside the scope at compile time
        {"name": "entry-any-pattern", "match": POD, "validate": {"message": "m", "foreach": [
            {"list": LIST, "anyPattern": [{"name": "c*"}]}]}},
        _rule("pattern-variable", {"name": "{{element.name}}"}),
        _rule("pattern-metadata", {"(metadata)": {"name": "x"}}),
        {"name": "pattern-and-deny", "match": POD, "validate": {"message": "m", "foreach": [
            {"list": LIST, "pattern": {"name": "c*"},
             "deny": {"conditions": {"all": [{"key": "{{element.name}}", "operator": "Equals", "value": "x"}]}}}]}},
        {"name": "two-entries", "match": POD, "validate": {"message": "m", "foreach": [
            {"list": LIST, "pattern": {"name": "c*"}}, {"list": INIT, "pattern": {"name": "i*"}}]}},
        _rule("pattern-not-a-map", "c*"),
    ]
    return pd._policy("crafted-foreach-pattern", rules)


def int_policy():
    """Outside the CPU cap: a string pattern that compares the number's text form."""
    return pd._policy("foreach-pattern-int", [_rule("port-glob", {"port": "?0"}),
                                              _rule("name-set", {"name": "?*"})])


def typing_policy():
    """The arms of the int-typing guard: |n| >= 2^53 under a number pattern, an int inside a nested
    list under a glob, and ints in a scalar list (the leaf that walks every element)."""
    return pd._policy("foreach-pattern-typing", [
        _rule("big", {"port": 80}),
        _rule("nested-glob", {"=(ports)": [{"containerPort": "8*"}]}),
        _rule("list-number", {"=(args)": [80]}),
        _rule("list-glob", {"=(args)": ["8*"]}),
    ])


def typing_resources():
    def pod(i, **container):
        return {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": f"t{i}", "namespace": "ns0"},
                "spec": {"containers": [{"name": "c0", "port": 80}, dict({"name": "c1", "port": 80}, **container)]}}
    return [
        pod(0),
        pod(1, port=1 << 53),
        pod(2, port=(1 << 53) - 1),
        pod(3, port=-(1 << 53)),
        pod(4, ports=[{"containerPort": 8443.5}, {"containerPort": 8443}]),
        pod(5, ports=[{"containerPort": 8443.5}, {"containerPort": 80.25}]),
        pod(6, ports=[{"containerPort": 9.5}]),
        pod(7, args=[80, 80]),
        pod(8, args=[80, 1 << 53]),
        pod(9, args=[80.0, 8.5]),
        pod(10, args=[80.5, 8443]),
        pod(11, args=[80.5, 8.25]),
    ]


def crafted_resources(n, float_ports=False):
    """foreach_data.crafted_resources with `ports` on the containers: container j of resource i
    gets (i + j) % 4 entries, entry t {"containerPort": 80 or 8443, "name": "p<t>"}; none: no key."""
    out = fd.crafted_resources(n)
    for i, res in enumerate(out):
        cs = res["spec"].get("containers")
        for j, c in enumerate(cs if isinstance(cs, list) else [cs]):
            if not isinstance(c, dict):
                continue
            k = (i + j) % 4
            if k:
                c["ports"] = [{"containerPort": 80 if (i + j + t) % 5 else 8443, "name": f"p{t}"} for t in range(k)]
            if float_ports:
                c["port"] = c["port"] / 160  # 0.5, 50.5
    return out


def on_device(rule) -> bool:
    return fd.is_foreach(rule) and rule["name"] not in CPU_RULES


# ---- the typing of numbers: which pattern strings compare a number's text form
def _atom_sensitive(orc, atom: str) -> bool:
    """One '&' part of one '|' alternative of a string pattern: after the operator, an operand that
    parses as a quantity is compared as a quantity (int64 n and float64(n) agree); anything else
    is matched against the number's text form, unless it matches everything."""
    op = orc.operator(atom)
    parts = [atom]
    if op == "-":
        parts = atom.split("-")
    elif op == "!-":
        parts = atom.split("!-")
    elif op:
        parts = [atom[len(op):]]
    for p in parts:
        p = p.strip()
        if p and set(p) <= {"*"}:
            continue
        if orc.quantity(p) is None:
            return True
    return False


def sensitive(orc, pattern) -> bool:
    if not isinstance(pattern, str):
        return False  # a number, bool or null pattern
    return any(_atom_sensitive(orc, c.strip()) for a in pattern.split("|") for c in a.strip().split("&"))


_ANCHOR = re.compile(r"^[<=X^+]?\((.*)\)$")


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def meets_int(orc, pattern, value) -> bool:
    """Conservative, as the device is: some leaf of the pattern that compares text forms stands
    over an int-typed value of the element (whatever the walk's order would reach first)."""
    if isinstance(pattern, dict):
        if not isinstance(value, dict):
            return False
        for k, p in pattern.items():
            key = _ANCHOR.sub(r"\1", k)
            if key in value and meets_int(orc, p, value[key]):
                return True
        return False
    if isinstance(pattern, list):
        if not pattern:
            return False
        if isinstance(pattern[0], (dict, list)):
            return isinstance(value, list) and any(meets_int(orc, pattern[0], v) for v in value)
        pattern = pattern[0]
    vals = value if isinstance(value, list) else [value]
    return any(_is_int(v) and (abs(v) >= 1 << 53 or sensitive(orc, pattern)) for v in vals)


class Expected:
    """The decomposition for one policy over resources: statuses and, per FAIL / ERROR pair of a
    device rule, the deciding element, the element-relative failing path (FAIL), the pattern
    error's text (the oracle's `msg`) and the rule message."""

    def __init__(self, orc, policy, resources):
        self.orc = orc
        self.lenient = cond_model.Model(orc)
        self.model = foreach_model.Model(orc)
        ost, _ = orc.validate_batch(json.dumps([fd.match_policy(policy)]), json.dumps(resources), nthreads=8)
        ost = ost.copy()
        ost[ost == 7] = CPU
        rules = policy["spec"]["rules"]
        self.rules, self.resources = rules, resources
        self.status = ost.copy()
        self.elem, self.path, self.err, self.messages, self.all_codes = {}, {}, {}, {}, {}
        self._memo = {}
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
                v, el, detail = self.foreach(rule, res, (ri, k))
                self.status[ri, k] = STATUS[v]
                if v in ("fail", "error"):
                    self.elem[(ri, k)] = el
                    self.err[(ri, k)] = detail["msg"]
                    if v == "fail":
                        self.path[(ri, k)] = detail["path"]
                    self.messages[(ri, k)] = HEAD + self.build_error_message(rule, res, detail, el)
                elif v in ("pass", "skip"):
                    self.messages[(ri, k)] = foreach_model.PASSED if v == "pass" else foreach_model.SKIPPED

    def element(self, rule, entry, resource, element):
        """validate() on one element: (code, MatchPattern's result)."""
        pre = entry.get("preconditions")
        if pre is not None:
            v = self.model.lenient.preconditions(pre, (resource, element))
            if v == cond_model.UNKNOWN:
                return "cpu", None
            if v is False:
                return "skip", None
        pat = entry["pattern"]
        if meets_int(self.orc, pat, element):
            return "cpu", None
        key = (json.dumps(element, sort_keys=True), json.dumps(pat, sort_keys=True))
        got = self._memo.get(key)
        if got is None:
            got = self._memo[key] = self.orc.match_pattern(json.dumps(element), json.dumps(pat), res_mode=0)
        assert "panic" not in got, got
        if not got["set"]:
            return "pass", None
        if got["skip"]:
            return "skip", None
        return ("error" if got["path"] == "" else "fail"), got

    def foreach(self, rule, resource, at=None):
        entry = rule["validate"]["foreach"][0]
        state, elems = self.model.elements(entry["list"], resource)
        if state == "cpu":
            return "cpu", None, None
        codes = [self.element(rule, entry, resource, e) for e in elems]
        if at is not None:
            self.all_codes[at] = [c for c, _ in codes]
        applied = 0
        for i, (c, detail) in enumerate(codes):
            if c == "skip":
                continue
            if c == "pass":
                applied += 1
                continue
            return c, i, detail
        return ("pass", None, None) if applied else ("skip", None, None)

    def build_error_message(self, rule, resource, detail, el):
        """buildErrorMessage (validation.go:510-534) in the element's context."""
        name, msg = rule["name"], rule["validate"].get("message", "")
        tail = f"failed at path {detail['path']}" if detail["path"] else f"execution error: {detail['msg']}"
        if not msg:
            return f"validation error: rule {name} {tail}"
        entry = rule["validate"]["foreach"][0]
        _, elems = self.model.elements(entry["list"], resource)
        m = self.model.strict.message(rule, (resource, elems[el]), "fail")
        return f"validation error: {m if m.endswith('.') else m + '.'} Rule {name} {tail}"

    def counts(self):
        c = np.zeros((self.status.shape[0], 8), dtype=np.int64)
        for s in range(7):
            c[:, s] = (self.status == s).sum(axis=1)
        return c

    def device_pairs(self, rows=None):
        rows = [ri for ri, r in enumerate(self.rules) if on_device(r)] if rows is None else rows
        st = self.status[rows]
        return st[st != NOMATCH]

    def check_honest(self, full: bool):
        """Conditions on the inputs, from the model alone: at most 10 % of the matched device pairs
        are CPU; at the full size the condition-anchor rule yields all five statuses, with an
        ERROR element both before and after a FAIL one; FAIL is decided by first, middle and last
        elements; failing paths reach into the second and third port."""
        pairs = self.device_pairs()
        if len(pairs) >= 100:
            assert (pairs == CPU).sum() * 10 <= len(pairs), ((pairs == CPU).sum(), len(pairs))
        names = [r["name"] for r in self.rules]
        ti = names.index("tier-image")
        seen = set()
        for (ri, k), cs in self.all_codes.items():
            if ri == ti and "fail" in cs and "error" in cs:
                fails = [i for i, c in enumerate(cs) if c == "fail"]
                errs = [i for i, c in enumerate(cs) if c == "error"]
                if min(errs) < max(fails):
                    seen.add("before")
                if max(errs) > min(fails):
                    seen.add("after")
        if len(self.resources) in (63, 65, 257, 513):
            assert {"before", "after"} <= seen, seen
        if not full:
            return
        for s in (PASS, FAIL, ERROR, SKIP, CPU):
            assert (self.device_pairs([ti]) == s).any(), s
        nl = names.index("no-latest")
        where = set()
        for k, res in enumerate(self.resources):
            if self.status[nl, k] == FAIL:
                cs = res["spec"]["containers"]
                n_el = len(cs) if isinstance(cs, list) else 1
                e = self.elem[(nl, k)]
                where.add("first" if e == 0 else "last" if e == n_el - 1 else "middle")
        assert where >= {"first", "middle", "last"}, where
        paths = set(self.path.values())
        assert {"/ports/", "/ports/0/containerPort/", "/ports/1/containerPort/", "/ports/2/containerPort/"} <= paths, \
            sorted(paths)
