"""Shared data of the tests of foreach rules of several entries (test_foreach_chain_cpu.py,
test_gpu_foreach_chain.py): the golden cases, a crafted policy, its resources and the expected
side. The expectation is the decomposition of foreach_data.py with foreach_chain_model.py in the
last step: the oracle for match / exclude, cond_model.py for the rule's own preconditions, the
chain model for the entries.

The cases the crafted set is built around (CASES: name -> what `Expected.check_cases` looks for):
  leak-resolves        an init container lacks imagePullPolicy and the last container has it: the
                       deny entry of `pull-policy` resolves (PASS or FAIL) where it would be ERROR;
  leak-pass-to-fail    the same leaked value opens the entry gate of `gated-pull`: FAIL where the
                       rule would PASS;
  nested-merge         `nested-merge`: securityContext.capabilities comes from the base while
                       securityContext.privileged comes from the element;
  array-replaced       `array-replaced`: an element's `args` replaces the base's, it is not merged;
  three-entries        `three-entries`: the third entry reads keys leaked by the first two;
  first-not-found      entry 1's list is missing: nothing leaks;
  first-empty          entry 1's list is []: nothing leaks;
  first-single-map     entry 1's list is one map: it is the one element, and it leaks;
  skip-then-pass       `skip-then-pass`: every element of entry 1 is skipped, entry 2 passes: PASS;
  all-skipped          every entry is skipped or empty: SKIP;
  decisive-before-oos  entry 1 decides while entry 2's list is out of scope: entry 1's status;
  pass-then-oos        entry 1 passes and entry 2's list is out of scope: CPU;
  mixed                `mixed`: a pattern entry and a deny entry in one rule, each deciding somewhere;
  pattern-sees-raw     `pattern-raw`: `tier` is absent in the raw element and present in the leak:
                       the entry precondition on it holds, the pattern on it fails;
  routed               `seventeen-entries` and `any-pattern-entry` stay (CPU, "foreach").
"""
from __future__ import annotations

import copy
import json
import os

import numpy as np

import cond_model
import foreach_chain_model
import foreach_data as fd
import precond_data as pd

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES_GOLDEN = json.load(open(os.path.join(GOLDEN, "foreach_chain.json")))["cases"]

PASS, FAIL, WARN, ERROR, SKIP, NOMATCH, CPU = range(7)
STATUS = fd.STATUS
NOT_MET = pd.NOT_MET
POD = pd.POD
NONE = 0xFFFFFFFF
C = "request.object.spec.containers"
I = "request.object.spec.initContainers"
E = "request.object.spec.ephemeralContainers"
IPP = "{{element.imagePullPolicy}}"
CPU_RULES = ("seventeen-entries", "any-pattern-entry")
# chain rules with a pattern entry (no host fold)
PATTERN_RULES = ("mixed", "pattern-raw")
CASES = ("leak-resolves", "leak-pass-to-fail", "nested-merge", "array-replaced", "three-entries", "first-not-found",
         "first-empty", "first-single-map", "skip-then-pass", "all-skipped", "decisive-before-oos", "pass-then-oos",
         "mixed", "pattern-sees-raw", "routed")


def _all(*conds):
    return {"conditions": {"all": [{"key": k, "operator": op, "value": v} for k, op, v in conds]}}


def _rule(name, entries, message="denied", pre=None):
    r = {"name": name, "match": POD, "validate": {"message": message, "foreach": entries}}
    if pre is not None:
        r["preconditions"] = pre
    return r


def crafted_policy():
    never = {"list": C, "deny": _all((IPP, "Equals", "Never"))}
    always = {"list": I, "deny": _all((IPP, "Equals", "Always"))}
    passes = {"list": C, "deny": _all(("{{element.name}}", "Equals", "no-such-name"))}
    rules = [
        # a rule of one entry: its set is the one the first entry of `pull-policy` uses
        _rule("single-pull", [copy.deepcopy(never)]),
        _rule("pull-policy", [copy.deepcopy(never), copy.deepcopy(always)], "policy " + IPP + " of {{element.name}}"),
        # the same second entry behind another list: another leak context, another set
        _rule("pull-policy-after-ephemeral", [{"list": E, "deny": _all((IPP, "Equals", "Never"))}, copy.deepcopy(always)]),
        _rule("gated-pull", [copy.deepcopy(passes),
                             {"list": I, "preconditions": {"all": [{"key": IPP, "operator": "Equals", "value": "Always"}]},
                              "deny": _all(("{{element.image}}", "Equals", "*:latest"))}],
              "latest image {{element.image}} pulled {{element.imagePullPolicy}}"),
        _rule("nested-merge", [copy.deepcopy(passes),
                               {"list": I, "deny": _all(("{{element.securityContext.capabilities.level}}", "Equals", "high"),
                                                        ("{{element.securityContext.privileged}}", "Equals", True))}],
              "{{element.name}}: {{element.securityContext.capabilities.level}}/{{element.securityContext.privileged}}"),
        _rule("array-replaced", [copy.deepcopy(passes), {"list": I, "deny": _all(("{{element.args[1]}}", "Equals", "b"))}],
              "second argument of {{element.name}}"),
        _rule("three-entries", [copy.deepcopy(passes),
                                {"list": I, "deny": _all(("{{element.name}}", "Equals", "no-such-name"))},
                                {"list": E, "deny": _all((IPP, "Equals", "Always"), ("{{element.stage}}", "Equals", "init"))}],
              "{{element.name}} in stage {{element.stage}}"),
        _rule("skip-then-pass", [{"list": C, "preconditions": {"all": [{"key": "{{element.name}}", "operator": "Equals", "value": "nope"}]},
                                  "deny": _all(("{{element.image}}", "Equals", "*"))},
                                 {"list": I, "deny": _all(("{{element.image}}", "Equals", "bad/*"))}]),
        _rule("mixed", [{"list": C, "pattern": {"image": "!*:latest"}},
                        {"list": I, "deny": _all(("{{element.image}}", "Equals", "*:latest"))}],
              "image of {{element.name}} is tagged latest"),
        _rule("pattern-raw", [copy.deepcopy(passes),
                              {"list": I, "preconditions": {"all": [{"key": "{{element.tier}}", "operator": "Equals", "value": "gold"}]},
                               "pattern": {"tier": "gold"}}], "tier {{element.tier}} of {{element.name}}"),
        _rule("behind-preconditions", [copy.deepcopy(never), copy.deepcopy(always)],
              pre={"all": [{"key": fd.APP, "operator": "NotEquals", "value": "db"}]}),
        # the same chain twice
        _rule("shared", [copy.deepcopy(never), copy.deepcopy(always)], "shared"),
        # outside the scope at compile time
        _rule("seventeen-entries", [copy.deepcopy(never) for _ in range(17)]),
        _rule("any-pattern-entry", [copy.deepcopy(never), {"list": I, "anyPattern": [{"name": "i*"}]}]),
        {"name": "plain-pattern", "match": POD, "validate": {"message": "tagged", "pattern": pd.IMAGE_TAG}},
    ]
    return pd._policy("crafted-foreach-chain", rules)


COUNTS = (0, 1, 2, 3, 5, 33)


def _container(i, j):
    c = {"name": f"c{j}", "image": f"reg{(i + j) % 3}.io/app{j}:" + ("latest" if (i * 7 + j * 3) % 11 == 0 else "v1"),
         "tier": "gold" if (i + j) % 3 == 0 else "silver"}
    if (i + 2 * j) % 13 != 0:
        c["imagePullPolicy"] = "Never" if (i * 5 + j) % 29 == 0 else ("Always" if (i + j) % 2 == 0 else "IfNotPresent")
    if (i + j) % 5 != 0:
        c["securityContext"] = {"capabilities": {"level": "high" if (i + j) % 2 else "low"}, "privileged": False}
    if (i + j) % 2 == 0:
        c["args"] = ["a", "b", "c"]
    return c


def _init(i, t):
    c = {"name": f"init{t}", "image": f"reg{i % 3}.io/init:" + ("latest" if (i + t) % 5 == 0 else "v1"), "stage": "init"}
    if (i + t) % 3 == 0:
        c["imagePullPolicy"] = "Always" if (i + t) % 2 == 0 else "IfNotPresent"
    if (i + t) % 4 != 1:
        c["securityContext"] = {"privileged": (i + t) % 2 == 0}
    if (i + t) % 3 == 1:
        c["args"] = ["x"]
    if (i + t) % 7 == 0:
        c["tier"] = "gold"
    return c


def crafted_resources(n):
    """Pods whose container counts are 300 and 70 (the first two: their segments straddle wave and
    workgroup boundaries at every size) and then cycle through 0, 1, 2, 3, 5, 33, with init
    container lists of other lengths (130 on the first, then 0 to 3: the entry kernels' grids
    differ) and an ephemeral container on some; either list missing, [], a single map, a scalar or
    a non-map element, a null inside an element on some; a few other kinds."""
    out = []
    for i in range(n):
        cnt = 300 if i == 0 else 70 if i == 1 else COUNTS[(i - 2) % len(COUNTS)]
        cs = [_container(i, j) for j in range(cnt)]
        spec = {"containers": cs}
        if i % 19 == 4:
            del spec["containers"]
        elif i % 23 == 6:
            spec["containers"] = _container(i, 0)
        elif i % 29 == 8:
            spec["containers"] = []
        elif i % 43 == 9 and cs:
            cs[len(cs) // 2] = "not-a-map"
        elif i % 47 == 10 and cs:
            cs[-1]["tier"] = None
        ni = 130 if i == 0 else i % 4
        if ni:
            spec["initContainers"] = [_init(i, t) for t in range(ni)]
        if i % 11 == 3:
            spec["initContainers"] = []
        elif i % 13 == 5:
            spec["initContainers"] = "none"
        elif i % 17 == 7:
            spec["initContainers"] = _init(i, 0)
        if i % 5 == 2:
            spec["ephemeralContainers"] = [{"name": "dbg", "image": "busybox"}]
        elif i % 10 == 7:
            spec["ephemeralContainers"] = [{"name": "dbg", "image": "busybox", "stage": "debug"}]
        labels = {"app": ["web", "db", "cache", "other"][i % 4]}
        meta = {"name": f"p{i}", "namespace": f"ns{i % 3}", "labels": labels}
        if i % 31 == 3:
            del meta["labels"]
        kind = "Deployment" if i % 9 == 5 else "Pod"
        out.append({"apiVersion": "apps/v1" if kind == "Deployment" else "v1", "kind": kind, "metadata": meta, "spec": spec})
    return out


def is_chain(rule) -> bool:
    return fd.is_foreach(rule) and len(rule["validate"]["foreach"]) > 1


def on_device(rule) -> bool:
    return fd.is_foreach(rule) and rule["name"] not in CPU_RULES


class Expected:
    """The decomposition for one policy over resources: statuses; per FAIL / ERROR pair of a device
    foreach rule the deciding entry and element, the failing path and pattern error where a pattern
    entry decided; messages; and the fold before match and the rule's preconditions (`fold`,
    `fold_entry`, `fold_elem`: what kv_batch_foreach_chain_fold gives for the rule's chain)."""

    def __init__(self, orc, policy, resources):
        self.lenient = cond_model.Model(orc)
        self.model = foreach_chain_model.Model(orc)
        ost, _ = orc.validate_batch(json.dumps([fd.match_policy(policy)]), json.dumps(resources), nthreads=8)
        ost = ost.copy()
        ost[ost == 7] = CPU
        rules = policy["spec"]["rules"]
        self.rules, self.resources = rules, resources
        self.status = ost.copy()
        self.gated = np.zeros_like(ost, dtype=bool)
        self.messages, self.entry, self.elem, self.path, self.err = {}, {}, {}, {}, {}
        self.fold = np.full(ost.shape, 255, dtype=np.uint8)
        self.fold_entry = np.full(ost.shape, NONE, dtype=np.uint32)
        self.fold_elem = np.full(ost.shape, NONE, dtype=np.uint32)
        for ri, rule in enumerate(rules):
            if not fd.is_foreach(rule):
                continue
            for k, res in enumerate(resources):
                if not on_device(rule):
                    if ost[ri, k] != NOMATCH:
                        self.status[ri, k] = CPU
                    continue
                v, en, el, msgs, detail = self.model.chain(rule, res)
                self.fold[ri, k] = STATUS[v]
                if v in ("fail", "error"):
                    self.fold_entry[ri, k], self.fold_elem[ri, k] = en, el
                if ost[ri, k] == NOMATCH:
                    continue
                assert ost[ri, k] == PASS, (rule["name"], k, ost[ri, k])
                if "preconditions" in rule:
                    p = self.lenient.preconditions(rule["preconditions"], res)
                    if p == cond_model.UNKNOWN:
                        self.status[ri, k] = CPU
                        continue
                    if p is False:
                        self.status[ri, k] = SKIP
                        self.gated[ri, k] = True
                        self.messages[(ri, k)] = [NOT_MET]
                        continue
                self.status[ri, k] = STATUS[v]
                if msgs is not None:
                    self.messages[(ri, k)] = msgs
                if v in ("fail", "error"):
                    self.entry[(ri, k)], self.elem[(ri, k)] = en, el
                    if detail is not None:
                        self.err[(ri, k)] = detail["msg"]
                        if v == "fail":
                            self.path[(ri, k)] = detail["path"]

    def counts(self):
        c = np.zeros((self.status.shape[0], 8), dtype=np.int64)
        for s in range(7):
            c[:, s] = (self.status == s).sum(axis=1)
        return c

    def chain_pairs(self):
        """The statuses of the matched pairs of the device rules of several entries."""
        rows = [ri for ri, r in enumerate(self.rules) if on_device(r) and is_chain(r)]
        st = self.status[rows]
        return st[st != NOMATCH]

    def check_cases(self):
        """Conditions on the inputs, from the models alone: the chain rules' pairs include all five
        statuses, at most 15 % of them CPU, and every case of CASES occurs. `without`: the chain
        model with the leak switched off (every entry sees its raw element)."""
        pairs = self.chain_pairs()
        for s in (PASS, FAIL, ERROR, SKIP, CPU):
            assert (pairs == s).any(), s
        assert (pairs == CPU).sum() * 100 <= 15 * len(pairs), ((pairs == CPU).sum(), len(pairs))
        names = [r["name"] for r in self.rules]
        m = self.model

        def without(rule, res):
            b = m.leak
            m.leak = False
            try:
                return m.chain(rule, res)
            finally:
                m.leak = b

        def state(res, key):
            return m.elements("request.object.spec." + key, res)

        seen = set()
        pods = [r for r in self.resources if r["kind"] == "Pod"]
        pp, gp = self.rules[names.index("pull-policy")], self.rules[names.index("gated-pull")]
        nm, ar = self.rules[names.index("nested-merge")], self.rules[names.index("array-replaced")]
        te, sp = self.rules[names.index("three-entries")], self.rules[names.index("skip-then-pass")]
        mx, pr = self.rules[names.index("mixed")], self.rules[names.index("pattern-raw")]
        mixed_by = set()
        for res in pods:
            cst, cel = state(res, "containers")
            ist, iel = state(res, "initContainers")
            got, base = m.chain(pp, res), without(pp, res)
            if base[0] == "error" and base[1] == 1 and got[0] in ("pass", "fail"):
                seen.add("leak-resolves")
            if base[0] == "error" and base[1] == 1 and got[0] == "error" and ist == "ok" and iel:
                if cst == "empty":
                    seen.add("first-not-found")
                if cst == "ok" and not cel:
                    seen.add("first-empty")
            if isinstance(res["spec"].get("containers"), dict) and base[:2] == ("error", 1) and got[0] != "error":
                seen.add("first-single-map")
            if got[0] in ("fail", "error") and got[1] == 0 and ist == "cpu":
                seen.add("decisive-before-oos")
            if got[0] == "cpu" and got[1] == 1 and cst == "ok":
                seen.add("pass-then-oos")
            if without(gp, res)[0] == "pass" and m.chain(gp, res)[0] == "fail":
                seen.add("leak-pass-to-fail")
            g = m.chain(nm, res)
            if g[0] == "fail":
                e = iel[g[2]]
                if "capabilities" not in e.get("securityContext", {}) and e.get("securityContext", {}).get("privileged") is True:
                    seen.add("nested-merge")
            g = m.chain(ar, res)
            if g[0] == "pass" and cst == "ok" and cel and "args" in cel[-1] and ist == "ok" and \
                    any(e.get("args") == ["x"] for e in iel):
                seen.add("array-replaced")
            if m.chain(te, res)[:2] == ("fail", 2):
                seen.add("three-entries")
            g = m.chain(sp, res)
            if g[0] == "pass" and cst == "ok" and cel:
                seen.add("skip-then-pass")
            if g[0] == "skip" and cst == "ok" and cel:
                seen.add("all-skipped")
            g = m.chain(mx, res)
            if g[0] == "fail":
                mixed_by.add(g[1])
            g = m.chain(pr, res)
            if g[0] == "fail" and g[1] == 1 and "tier" not in iel[g[2]] and without(pr, res)[0] != "fail":
                seen.add("pattern-sees-raw")
        if mixed_by == {0, 1}:
            seen.add("mixed")
        if all(n in names for n in CPU_RULES):
            seen.add("routed")
        assert seen == set(CASES), sorted(set(CASES) - seen)
