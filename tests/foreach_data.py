"""Shared data of the foreach tests (test_foreach_cpu.py, test_gpu_foreach.py): the golden cases,
the crafted rule set and its resources, and the expected side. The oracle reports foreach rules as
CPU, so the expectation is the decomposition of deny_data.py with the foreach model in the last step:

    expected(rule, res) = NOMATCH where the oracle gives NOMATCH for the same rule with its
    `validate` replaced by an always-passing pattern and `preconditions` deleted; else, from the
    rule's preconditions (cond_model.py): CPU where they are unknown, SKIP where they are false;
    else the foreach model (foreach_model.py).
"""
from __future__ import annotations

import copy
import json
import os

import numpy as np

import cond_model
import foreach_model
import precond_data as pd

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = json.load(open(os.path.join(GOLDEN, "foreach.json")))["cases"]

PASS, FAIL, WARN, ERROR, SKIP, NOMATCH, CPU = range(7)
STATUS = {"pass": PASS, "fail": FAIL, "error": ERROR, "skip": SKIP, "cpu": CPU}
NOT_MET = pd.NOT_MET
POD = pd.POD
ALWAYS = {"message": "always", "pattern": {"metadata": {"name": "?*"}}}
NO_ELEM = 0xFFFFFFFF

LIST = "request.object.spec.containers"
INIT = "request.object.spec.initContainers"
APP = "{{request.object.metadata.labels.app}}"
NS = "{{request.object.metadata.namespace}}"
# rules that stay on the CPU route with the flag on
CPU_RULES = ("two-entries", "entry-pattern", "entry-list-preconditions", "whole-element")


def crafted_policy():
    def rule(name, conditions, message="denied", pre=None, epre=None, lst=LIST):
        entry = {"list": lst, "deny": {"conditions": conditions}}
        if epre is not None:
            entry["preconditions"] = epre
        r = {"name": name, "match": POD, "validate": {"message": message, "foreach": [entry]}}
        if pre is not None:
            r["preconditions"] = pre
        return r
    latest = {"all": [{"key": "{{element.image}}", "operator": "Equals", "value": "*:latest"}]}
    rules = [
        # FAIL on the first, a middle and the last element, by resource
        rule("no-latest", latest, "image {{element.image}} of {{element.name}} in " + NS + " is denied"),
        # an unresolved string (ERROR) before and after a FAIL element; a message variable that
        # does not resolve on the element leaves the raw message
        rule("tier-denied", {"all": [{"key": "{{element.tier}}", "operator": "Equals", "value": "bad"}]},
             "tier {{element.tier}} / {{element.missing}}"),
        # a map operand (undecided: CPU) before and after a FAIL element
        rule("resources-class", {"any": [{"key": "{{element.resources}}", "operator": "Equals", "value": "big"}]}, ""),
        # entry preconditions gate c0: one-container resources are SKIP
        rule("gated", {"all": [{"key": "{{element.image}}", "operator": "Equals", "value": "reg0.io/*"}]},
             epre={"all": [{"key": "{{element.name}}", "operator": "NotEquals", "value": "c0"}]}),
        # the preconditions resolver: a missing tier is "", and only those elements are evaluated
        rule("gated-optional", {"any": [{"key": "{{element.name}}", "operator": "In", "value": ["c1", "c4", "c6?"]}]},
             epre={"any": [{"key": "{{element.tier}}", "operator": "Equals", "value": ""}]}),
        # both roots in one string, and a request.object string beside an element string
        rule("mixed-string", {"all": [{"key": NS + "/{{element.name}}", "operator": "Equals", "value": "ns1/c2"}]},
             "container {{element.name}} of " + NS),
        rule("both-roots", {"all": [{"key": APP, "operator": "Equals", "value": "web"},
                                    {"key": "{{element.port}}", "operator": "GreaterThan", "value": 1024}]}),
        # the old list form, a variable on the value side
        rule("old-form", [{"key": "c1", "operator": "Equals", "value": "{{element.name}}"},
                          {"key": "{{element.port}}", "operator": "LessThan", "value": 1000}]),
        # a rule-level precondition in front
        rule("behind-preconditions", copy.deepcopy(latest),
             pre={"all": [{"key": APP, "operator": "NotEquals", "value": "db"}]}),
        # another list (missing on most resources), and an index chain (a map: one element)
        rule("init-containers", {"all": [{"key": "{{element.image}}", "operator": "NotEquals", "value": "reg?.io/*"}]},
             lst=INIT),
        rule("first-container", {"all": [{"key": "{{element.name}}", "operator": "NotEquals", "value": "c0"}]},
             lst=LIST + "[0]"),
        # the same set twice
        rule("shared", copy.deepcopy(latest), "shared"),
        # constant blocks
        rule("constant-true", {"all": [{"key": "a", "operator": "Equals", "value": "a"}]}, "never allowed"),
        rule("constant-false", {"all": [{"key": 1, "operator": "GreaterThan", "value": 2},
                                        {"key": "{{element.name}}", "operator": "Equals", "value": "c0"}]}),
        # outside the scope at compile time
        {"name": "two-entries", "match": POD, "validate": {"message": "m", "foreach": [
            {"list": LIST, "deny": {"conditions": copy.deepcopy(latest)}},
            {"list": INIT, "deny": {"conditions": copy.deepcopy(latest)}}]}},
        {"name": "entry-pattern", "match": POD, "validate": {"message": "m", "foreach": [
            {"list": LIST, "pattern": {"name": "c*"}}]}},
        {"name": "entry-list-preconditions", "match": POD, "validate": {"message": "m", "foreach": [
            {"list": LIST, "preconditions": [{"key": "{{element.name}}", "operator": "Equals", "value": "c0"}],
             "deny": {"conditions": copy.deepcopy(latest)}}]}},
        rule("whole-element", {"all": [{"key": "{{element}}", "operator": "Equals", "value": "x"}]}),
        {"name": "plain-pattern", "match": POD, "validate": {"message": "tagged", "pattern": pd.IMAGE_TAG}},
    ]
    return pd._policy("crafted-foreach", rules)


COUNTS = (0, 1, 2, 3, 5, 64)


def _container(i, j):
    c = {"name": f"c{j}", "image": f"reg{(i + j) % 3}.io/app{j}:" + ("latest" if (i * 7 + j * 3) % 11 == 0 else "v1"),
         "port": 8080 if (i + j) % 4 == 0 else 80}
    if (i + 2 * j) % 13 != 0:
        c["tier"] = "bad" if (i + j) % 7 == 0 else "ok"
    c["resources"] = {"limits": {"cpu": "1"}} if (i * 3 + j) % 37 == 0 else ("big" if (i + j) % 5 == 0 else "small")
    return c


def crafted_resources(n):
    """Pods whose container counts are 300 and 70 (the first two: their segments straddle wave
    and workgroup boundaries at every size) and then cycle through 0, 1, 2, 3, 5, 64; the list
    missing, a single map, a scalar element, a null inside an element, a null list and a scalar
    list on some; initContainers on every fourth; labels missing on some; a few other kinds (the
    store order is permuted)."""
    out = []
    for i in range(n):
        cnt = 300 if i == 0 else 70 if i == 1 else COUNTS[(i - 2) % len(COUNTS)]
        cs = [_container(i, j) for j in range(cnt)]
        spec = {"containers": cs}
        if i % 19 == 4:
            del spec["containers"]
        elif i % 23 == 6:
            spec["containers"] = _container(i, 0)
        elif i % 43 == 8 and cs:
            cs[len(cs) // 2] = "not-a-map"
        elif i % 47 == 9 and cs:
            cs[-1]["tier"] = None
        elif i % 53 == 10:
            spec["containers"] = None
        elif i % 59 == 11:
            spec["containers"] = "none"
        if i % 4 == 1:
            spec["initContainers"] = [{"name": "init0", "image": f"reg{i % 3}.io/init:v1"},
                                      {"name": "init1", "image": "busybox" if i % 8 == 1 else "reg1.io/init:v2"}]
        labels = {"app": ["web", "db", "cache", "other"][i % 4]}
        meta = {"name": f"p{i}", "namespace": f"ns{i % 3}", "labels": labels}
        if i % 17 == 3:
            del meta["labels"]
        kind = "Deployment" if i % 9 == 5 else "Pod"
        out.append({"apiVersion": "apps/v1" if kind == "Deployment" else "v1", "kind": kind, "metadata": meta, "spec": spec})
    return out


def is_foreach(rule) -> bool:
    return "foreach" in (rule.get("validate") or {})


def on_device(rule) -> bool:
    return is_foreach(rule) and rule["name"] not in CPU_RULES


def match_policy(policy):
    p = copy.deepcopy(policy)
    for r in p["spec"]["rules"]:
        if is_foreach(r):
            r["validate"] = copy.deepcopy(ALWAYS)
            r.pop("preconditions", None)
    return p


class Expected:
    """The decomposition for one policy over resources: statuses, per device foreach pair the
    deciding element and its messages (ERROR pairs: one per unresolved string), and the fold
    before match and the rule's preconditions (`fold`, `fold_elem`: what kv_batch_foreach_fold
    gives for the rule's set)."""

    def __init__(self, orc, policy, resources):
        self.lenient = cond_model.Model(orc)
        self.model = foreach_model.Model(orc)
        ost, _ = orc.validate_batch(json.dumps([match_policy(policy)]), json.dumps(resources), nthreads=8)
        ost = ost.copy()
        ost[ost == 7] = CPU
        rules = policy["spec"]["rules"]
        self.rules, self.resources = rules, resources
        self.status = ost.copy()
        self.gated = np.zeros_like(ost, dtype=bool)
        self.messages, self.elem, self.codes = {}, {}, {}
        self.fold = np.full(ost.shape, 255, dtype=np.uint8)
        self.fold_elem = np.full(ost.shape, NO_ELEM, dtype=np.uint32)
        for ri, rule in enumerate(rules):
            if not is_foreach(rule):
                continue
            for k, res in enumerate(resources):
                if not on_device(rule):
                    if ost[ri, k] != NOMATCH:
                        self.status[ri, k] = CPU
                    continue
                v, el, msgs = self.model.foreach(rule, res)
                self.fold[ri, k] = STATUS[v]
                if v in ("fail", "error", "cpu") and el is not None:
                    self.fold_elem[ri, k] = el
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
                    self.elem[(ri, k)] = el

    def counts(self):
        c = np.zeros((self.status.shape[0], 8), dtype=np.int64)
        for s in range(7):
            c[:, s] = (self.status == s).sum(axis=1)
        return c

    def device_pairs(self):
        """The statuses of the matched pairs of the device foreach rules."""
        rows = [ri for ri, r in enumerate(self.rules) if on_device(r)]
        st = self.status[rows]
        return st[st != NOMATCH]

    def check_honest(self, full: bool):
        """A condition on the inputs, from the model alone: at most 10 % of the matched foreach
        pairs are CPU; at the full size every status occurs, FAIL is decided by the first, a middle
        and the last element, and an ERROR / an undecided element stands before and after a FAIL one."""
        pairs = self.device_pairs()
        if len(pairs) >= 100:
            assert (pairs == CPU).sum() * 10 <= len(pairs), ((pairs == CPU).sum(), len(pairs))
        if not full:
            return
        for s in (PASS, FAIL, ERROR, SKIP, CPU):
            assert (pairs == s).any(), s
        names = [r["name"] for r in self.rules]
        nl = names.index("no-latest")
        where = set()
        for k, res in enumerate(self.resources):
            if self.status[nl, k] == FAIL:
                cs = res["spec"]["containers"]
                n_el = len(cs) if isinstance(cs, list) else 1
                e = self.elem[(nl, k)]
                where.add("first" if e == 0 else "last" if e == n_el - 1 else "middle")
                if n_el > 1 and e == n_el - 1:
                    where.add("last-of-many")
        assert where >= {"first", "middle", "last", "last-of-many"}, where
        for name, other in (("tier-denied", "error"), ("resources-class", "cpu")):
            ri = names.index(name)
            seen = set()
            for res in self.resources:
                if res["kind"] != "Pod":
                    continue
                cs = [c for c, _ in self.model.codes(self.rules[ri], res)[1]]
                if "fail" in cs and other in cs:
                    seen.add("before" if cs.index(other) < cs.index("fail") else "after")
            assert seen == {"before", "after"}, (name, seen)
        g = self.status[names.index("gated")]
        one = np.array([x["kind"] == "Pod" and isinstance(x["spec"].get("containers"), list) and
                        len(x["spec"]["containers"]) == 1 and isinstance(x["spec"]["containers"][0], dict) and
                        not foreach_model.has_null(x["spec"]["containers"][0]) for x in self.resources])
        assert one.any() and (g[one] == SKIP).all()  # every element gated
        assert self.gated[names.index("behind-preconditions")].any()
