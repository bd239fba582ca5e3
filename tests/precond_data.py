"""Shared data of the precondition tests (test_preconditions_cpu.py, test_gpu_preconditions.py):
the golden condition rows as a policy, the crafted rule set and its resources, and the expected
side. The oracle reports rules with preconditions as CPU, so the expectation is a decomposition:

    expected(rule, res) = NOMATCH where the oracle gives NOMATCH for the same rule with
    `preconditions` deleted; else CPU where the model (cond_model.py) says "unknown"; else SKIP
    where the model says the preconditions are false; else the oracle's status, path and message
    for the stripped rule.
"""
from __future__ import annotations

import copy
import json
import os

import numpy as np

import cond_model

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CONDITIONS = json.load(open(os.path.join(GOLDEN, "conditions.json")))
ROWS = [r for r in CONDITIONS["rows"] if r["in_scope"]]
CLI_CASE = json.load(open(os.path.join(GOLDEN, "preconditions_cli.json")))

PASS, FAIL, WARN, ERROR, SKIP, NOMATCH, CPU = range(7)
NOT_MET = "preconditions not met"
POD = {"resources": {"kinds": ["Pod"]}}


def _policy(name, rules):
    return {"apiVersion": "kyverno.io/v1", "kind": "ClusterPolicy", "metadata": {"name": name},
            "spec": {"validationFailureAction": "audit", "background": False, "rules": rules}}


# ------------------------------------------------------------------ golden table end to end
def golden_var_in_value(i: int) -> bool:
    """Rows whose variable side is the value: every third row with a scalar value (a list value on
    the resource would be an array operand, outside the scope)."""
    return i % 3 == 2 and not isinstance(ROWS[i]["value"], list)


def golden_policy():
    """One rule per in-scope golden row: the row's key (or value) comes from data.c<i>."""
    rules = []
    for i, row in enumerate(ROWS):
        var = "{{request.object.data.c%d}}" % i
        cond = {"key": row["key"], "operator": row["operator"], "value": var} if golden_var_in_value(i) else \
               {"key": var, "operator": row["operator"], "value": row["value"]}
        rules.append({"name": f"row-{i}", "match": POD, "preconditions": {"all": [cond]},
                      "validate": {"message": "golden row", "pattern": {"kind": "Pod"}}})
    return _policy("golden-conditions", rules)


def golden_resources(n=257):
    """Even resources carry the `data` map with every operand; odd ones no `data` at all, so every
    variable resolves to "" and neighbouring lanes disagree."""
    data = {f"c{i}": (row["value"] if golden_var_in_value(i) else row["key"]) for i, row in enumerate(ROWS)}
    out = []
    for k in range(n):
        r = {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": f"g{k}", "namespace": "default"},
             "spec": {"containers": [{"name": "c", "image": "nginx:1"}]}}
        if k % 2 == 0:
            r["data"] = data
        out.append(r)
    return out


def golden_expected(model, n=257):
    """[rule][res]: PASS / SKIP from the golden Result on even resources, from the model on odd."""
    exp = np.zeros((len(ROWS), n), dtype=np.uint8)
    for i, row in enumerate(ROWS):
        if golden_var_in_value(i):
            odd = model.evaluate(row["key"], row["operator"], "")
        else:
            odd = model.evaluate("", row["operator"], row["value"])
        exp[i, 0::2] = PASS if row["result"] else SKIP
        exp[i, 1::2] = PASS if odd else SKIP
    return exp


# ------------------------------------------------------------------ crafted parity
TIER = "{{request.object.metadata.labels.tier}}"
APP = "{{request.object.metadata.labels.app}}"
ZONES = "{{request.object.spec.zones}}"
PRIO = "{{request.object.metadata.labels.prio}}"
IMAGE_TAG = {"spec": {"containers": [{"image": "*:*"}]}}
SHARED = {"all": [{"key": APP, "operator": "AnyIn", "value": ["web", "db"]}]}


def crafted_policy():
    def rule(name, pre, validate, match=POD):
        r = {"name": name, "match": match, "validate": validate}
        if pre is not None:
            r["preconditions"] = pre
        return r
    rules = [
        rule("any-only", {"any": [{"key": TIER, "operator": "Equals", "value": "t1*"},
                                  {"key": APP, "operator": "In", "value": ["web", "cache"]}]},
             {"message": "images need a tag", "pattern": IMAGE_TAG}),
        rule("all-only", {"all": [{"key": TIER, "operator": "NotEquals", "value": "t5"},
                                  {"key": TIER, "operator": "AnyNotIn", "value": ["t6", "t7?"]}]},
             {"message": "names", "pattern": {"spec": {"containers": [{"name": "c*"}]}}}),
        rule("any-all-array", {"any": [{"key": APP, "operator": "Equals", "value": "web"},
                                       {"key": ZONES, "operator": "Equals", "value": "z1"}],
                               "all": [{"key": TIER, "operator": "NotIn", "value": ["t2", "t3", "t40"]}]},
             {"message": "tagged", "pattern": IMAGE_TAG}),
        rule("old-form", [{"key": PRIO, "operator": "GreaterThanOrEquals", "value": 2},
                          {"key": APP, "operator": "NotEquals", "value": ""}],
             {"message": "priority", "pattern": {"spec": {"priority": "<6"}}}),
        rule("empty-list", [], {"message": "tagged", "pattern": IMAGE_TAG}),
        rule("empty-map", {}, {"message": "tagged", "pattern": IMAGE_TAG}),
        rule("one-string-thrice", {"all": [{"key": TIER, "operator": "NotEquals", "value": "t10"},
                                           {"key": TIER, "operator": "NotEquals", "value": "t11"},
                                           {"key": TIER, "operator": "AllNotIn", "value": ["t12", "t13", "t6?"]}]},
             {"message": "tagged", "pattern": IMAGE_TAG}),
        rule("unknown-operator", {"all": [{"key": TIER, "operator": "Resembles", "value": "t1"}]},
             {"message": "tagged", "pattern": IMAGE_TAG}),
        rule("with-pattern-variable", {"all": [{"key": APP, "operator": "Equals", "value": "web"}]},
             {"message": "own namespace", "pattern": {"spec": {"serviceAccountName": "{{request.object.metadata.namespace}}"}}}),
        rule("any-pattern", {"any": [{"key": TIER, "operator": "In", "value": "t2*"},
                                     {"key": PRIO, "operator": "LessThan", "value": "3"}]},
             {"message": "host network or nginx",
              "anyPattern": [{"spec": {"hostNetwork": False}}, {"spec": {"containers": [{"image": "nginx*"}]}}]}),
        rule("shared-a", SHARED, {"message": "tagged", "pattern": IMAGE_TAG}),
        rule("shared-b", copy.deepcopy(SHARED), {"message": "names", "pattern": {"spec": {"containers": [{"name": "?"}]}}}),
        rule("conditional-anchor", {"any": [{"key": APP, "operator": "Equals", "value": "web"},
                                            {"key": "db", "operator": "Equals", "value": APP}]},
             {"message": "host network pods", "pattern": {"spec": {"(hostNetwork)": True, "priority": "<5"}}}),
        rule("in-string", {"all": [{"key": "{{request.object.metadata.namespace}}/" + APP, "operator": "Equals",
                                    "value": "ns1/*"}]},
             {"message": "tagged", "pattern": IMAGE_TAG}),
        rule("array-in-all", {"all": [{"key": ZONES, "operator": "NotEquals", "value": "z0"}]},
             {"message": "tagged", "pattern": IMAGE_TAG}),
        # one string in both lists, another string's condition between them in list order: the
        # gate's entries go by string across `any` and `all` together
        rule("one-string-any-and-all", {"any": [{"key": TIER, "operator": "In", "value": ["t2*", "t30"]},
                                                {"key": APP, "operator": "Equals", "value": "db"}],
                                        "all": [{"key": TIER, "operator": "NotEquals", "value": "t21"}]},
             {"message": "tagged", "pattern": IMAGE_TAG}),
        rule("no-preconditions", None, {"message": "tagged", "pattern": IMAGE_TAG}),
    ]
    return _policy("crafted-preconditions", rules)


def crafted_resources(n):
    """>= 70 distinct tier labels once n allows (outcome ids cross the 32- and 64-bit words of the
    bit planes), containers of varying shape and a few other kinds (the store order is permuted),
    labels that are numbers, bools or null, label maps missing, spec.zones an array on some."""
    out = []
    for i in range(n):
        labels = {"tier": f"t{i % 83}", "app": ["web", "db", "cache", "other"][i % 4], "prio": str(i % 7)}
        if i % 11 == 3:
            labels["tier"] = [5, True, None, 2.5][(i // 11) % 4]
        if i % 13 == 5:
            labels["prio"] = i % 5
        if i % 17 == 7:
            del labels["app"]
        md = {"name": f"r{i}", "namespace": f"ns{i % 3}"}
        if i % 19 != 9:
            md["labels"] = labels
        cs = [{"name": "c" if k == 0 else f"c{k}", "image": ["nginx:1", "redis", "nginx", "busybox:2"][(i + k) % 4]}
              for k in range(1 + i % 3)]
        spec = {"containers": cs, "priority": i % 9, "serviceAccountName": f"ns{(i // 2) % 3}"}
        if i % 2:
            spec["hostNetwork"] = bool(i % 8 == 1)
        if i % 5 == 0:
            spec["zones"] = ["z1", "z2"]
        elif i % 5 == 1:
            spec["zones"] = "z1"
        elif i % 5 == 2:
            spec["zones"] = "z0"
        kind = "Deployment" if i % 23 == 11 else "Pod"
        out.append({"apiVersion": "apps/v1" if kind == "Deployment" else "v1", "kind": kind, "metadata": md, "spec": spec})
    return out


def strip_preconditions(policy):
    p = copy.deepcopy(policy)
    for r in p["spec"]["rules"]:
        r.pop("preconditions", None)
    return p


class Expected:
    """The decomposition for one policy over resources: statuses, and per FAIL / SKIP / ERROR pair
    the path and the message."""

    def __init__(self, orc, policy, resources):
        self.model = cond_model.Model(orc)
        stripped = strip_preconditions(policy)
        ost, _ = orc.validate_batch(json.dumps([stripped]), json.dumps(resources), nthreads=8)
        ost = ost.copy()
        ost[ost == 7] = CPU
        # the pinned gate order (preconditions before pattern substitution, after the CPU checks)
        # is not exercised by this data: no stripped pair is CPU
        assert not (ost == CPU).any(), np.argwhere(ost == CPU)[:5]
        rules = policy["spec"]["rules"]
        self.stripped, self.resources, self.rules = stripped, resources, rules
        self.status = ost.copy()
        self.gated = np.zeros_like(ost, dtype=bool)       # SKIP decided by the preconditions
        self.unknown = np.zeros_like(ost, dtype=bool)
        for ri, rule in enumerate(rules):
            if "preconditions" not in rule:
                continue
            for k, res in enumerate(resources):
                if ost[ri, k] == NOMATCH:
                    continue
                v = self.model.preconditions(rule["preconditions"], res)
                if v == cond_model.UNKNOWN:
                    self.status[ri, k] = CPU
                    self.unknown[ri, k] = True
                elif v is False:
                    self.status[ri, k] = SKIP
                    self.gated[ri, k] = True
        self._orc = orc
        self._cache = {}

    def detail(self, ri, k):
        """(path, message) of pair (rule, res) as the reference reports it."""
        if self.gated[ri, k]:
            return None, NOT_MET
        if k not in self._cache:
            self._cache[k] = self._orc.validate(self.stripped, self.resources[k])["rules"]
        x = self._cache[k][ri]
        return x.get("path"), x["message"]

    def counts(self):
        """[rule][8] histogram of the expected matrix."""
        c = np.zeros((self.status.shape[0], 8), dtype=np.int64)
        for s in range(7):
            c[:, s] = (self.status == s).sum(axis=1)
        return c
