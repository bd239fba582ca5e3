"""Shared data of the deny tests (test_deny_cpu.py, test_gpu_deny.py): the golden cases, the
crafted rule set and its resources, and the expected side. The oracle reports deny rules as CPU,
so the expectation is a decomposition:

    expected(rule, res) = NOMATCH where the oracle gives NOMATCH for the same rule with its
    `validate` replaced by an always-passing pattern and `preconditions` deleted; else, from the
    preconditions (cond_model.py): CPU where they are unknown, SKIP where they are false; else, from
    the deny model (deny_model.py): ERROR where a variable of the block does not resolve, CPU where
    the fold is undecided, FAIL where the conditions hold, PASS where they do not.
"""
from __future__ import annotations

import copy
import json
import os

import numpy as np

import cond_model
import deny_model
import precond_data as pd

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = json.load(open(os.path.join(GOLDEN, "deny.json")))["cases"]
# test/cli/test/simple of the reference (policy duration-test: four deny rules), as recorded for
# tests/test_cli.py
CLI_SIMPLE = next(c for c in json.load(open(os.path.join(GOLDEN, "cli.json")))["cases"]
                  if c["kind"] == "kyverno_test" and c["src"] == "test/cli/test/simple/test.yaml")

PASS, FAIL, WARN, ERROR, SKIP, NOMATCH, CPU = range(7)
STATUS = {"pass": PASS, "fail": FAIL, "error": ERROR}
NOT_MET = pd.NOT_MET
POD = pd.POD
ALWAYS = {"message": "always", "pattern": {"metadata": {"name": "?*"}}}

TIER, APP, ZONES, PRIO = pd.TIER, pd.APP, pd.ZONES, pd.PRIO
NS = "{{request.object.metadata.namespace}}"
SHARED = {"any": [{"key": APP, "operator": "AnyIn", "value": ["web", "db"]}]}
# rules whose block reads spec.zones, an array on some resources: the only ones that may be CPU
ARRAY_RULES = ("any-all-array", "error-beats-array")


def crafted_policy():
    def rule(name, conditions, message="denied", pre=None, match=POD):
        r = {"name": name, "match": match, "validate": {"message": message, "deny": {"conditions": conditions}}}
        if pre is not None:
            r["preconditions"] = pre
        return r
    rules = [
        rule("any-only", {"any": [{"key": TIER, "operator": "Equals", "value": "t1*"},
                                  {"key": APP, "operator": "In", "value": ["web", "cache"]}]},
             "tier " + TIER + " of " + NS + " is denied"),
        rule("all-only", {"all": [{"key": TIER, "operator": "NotEquals", "value": "t5"},
                                  {"key": TIER, "operator": "AnyNotIn", "value": ["t6", "t7?"]}]},
             # (a message variable the block does not read: where it does not resolve, the raw message)
             "app " + APP + " has a denied tier"),
        rule("any-all-array", {"any": [{"key": APP, "operator": "Equals", "value": "web"},
                                       {"key": ZONES, "operator": "Equals", "value": "z1"}],
                               "all": [{"key": TIER, "operator": "NotIn", "value": ["t2", "t3", "t40"]}]}),
        rule("old-form", [{"key": PRIO, "operator": "GreaterThanOrEquals", "value": 2},
                          {"key": APP, "operator": "NotEquals", "value": ""}], ""),
        rule("numeric", {"all": [{"key": "{{request.object.spec.priority}}", "operator": "GreaterThan", "value": 4}]},
             "priority {{request.object.spec.priority}} is above 4"),
        rule("one-string-thrice", {"all": [{"key": TIER, "operator": "NotEquals", "value": "t10"},
                                           {"key": TIER, "operator": "NotEquals", "value": "t11"},
                                           {"key": TIER, "operator": "AllNotIn", "value": ["t12", "t13", "t6?"]}]}),
        rule("unknown-operator", {"any": [{"key": TIER, "operator": "Resembles", "value": "t1"}]}),
        rule("constant-true", {"all": [{"key": "a", "operator": "Equals", "value": "a"}]}, "never allowed"),
        rule("constant-false", {"all": [{"key": 1, "operator": "GreaterThan", "value": 2},
                                        {"key": APP, "operator": "Equals", "value": "web"}]}),
        rule("variable-in-value", {"all": [{"key": "db", "operator": "Equals", "value": APP}]}),
        rule("shared-a", SHARED, "shared a"),
        rule("shared-b", copy.deepcopy(SHARED), "shared b"),
        rule("behind-preconditions", {"all": [{"key": TIER, "operator": "In", "value": ["t2*", "t3*"]}]},
             pre={"all": [{"key": PRIO, "operator": "LessThan", "value": "4"}]}),
        rule("masked-error", {"all": [{"key": APP, "operator": "NotEquals", "value": "db"}]},
             pre={"all": [{"key": APP, "operator": "AnyIn", "value": ["web", "db"]}]}),
        rule("error-beats-array", {"all": [{"key": APP, "operator": "NotEquals", "value": "cache"},
                                           {"key": ZONES, "operator": "Equals", "value": "z1"}]}),
        {"name": "plain-pattern", "match": POD, "validate": {"message": "tagged", "pattern": pd.IMAGE_TAG}},
    ]
    return pd._policy("crafted-deny", rules)


def crafted_resources(n):
    """precond_data.crafted_resources: >= 70 distinct tier labels, label maps missing on some and
    single labels on others (an error under the strict resolver), labels that are numbers, bools or
    null, spec.zones an array on some and absent on others, a few non-Pod kinds."""
    return pd.crafted_resources(n)


def is_deny(rule) -> bool:
    return "deny" in (rule.get("validate") or {})


def match_policy(policy):
    """Every deny rule with an always-passing pattern and no preconditions: what the oracle can
    say about a deny rule is whether it matches."""
    p = copy.deepcopy(policy)
    for r in p["spec"]["rules"]:
        if is_deny(r):
            r["validate"] = copy.deepcopy(ALWAYS)
            r.pop("preconditions", None)
    return p


class Expected:
    """The decomposition for one policy over resources: statuses, and per deny pair its message
    (ERROR pairs: every message the reference may give, one per unresolved string)."""

    def __init__(self, orc, policy, resources):
        self.lenient = cond_model.Model(orc)
        self.strict = deny_model.Model(orc)
        ost, _ = orc.validate_batch(json.dumps([match_policy(policy)]), json.dumps(resources), nthreads=8)
        ost = ost.copy()
        ost[ost == 7] = CPU
        rules = policy["spec"]["rules"]
        self.rules, self.resources = rules, resources
        self.status = ost.copy()
        self.gated = np.zeros_like(ost, dtype=bool)  # SKIP decided by the preconditions
        self.messages = {}                           # (rule, res) -> [message, ...]
        for ri, rule in enumerate(rules):
            if not is_deny(rule):
                continue
            block = rule["validate"]["deny"]["conditions"]
            for k, res in enumerate(resources):
                if ost[ri, k] == NOMATCH:
                    continue
                assert ost[ri, k] == PASS, (rule["name"], k, ost[ri, k])
                if "preconditions" in rule:
                    v = self.lenient.preconditions(rule["preconditions"], res)
                    if v == cond_model.UNKNOWN:
                        self.status[ri, k] = CPU
                        continue
                    if v is False:
                        self.status[ri, k] = SKIP
                        self.gated[ri, k] = True
                        self.messages[(ri, k)] = [NOT_MET]
                        continue
                v, errs = self.strict.deny(block, res)
                if v == "error":
                    self.status[ri, k] = ERROR
                    self.messages[(ri, k)] = errs
                elif v == deny_model.UNKNOWN:
                    self.status[ri, k] = CPU
                else:
                    self.status[ri, k] = STATUS[v]
                    self.messages[(ri, k)] = [self.strict.message(rule, res, v)]

    def counts(self):
        """[rule][8] histogram of the expected matrix."""
        c = np.zeros((self.status.shape[0], 8), dtype=np.int64)
        for s in range(7):
            c[:, s] = (self.status == s).sum(axis=1)
        return c

    def check_honest(self, full: bool):
        """What keeps the crafted test honest: CPU pairs only on the rules built with array
        operands, neighbouring lanes disagree; at the full size every status occurs."""
        names = [r["name"] for r in self.rules]
        for ri, n in enumerate(names):
            if n not in ARRAY_RULES:
                assert not (self.status[ri] == CPU).any(), n
        if self.status.shape[1] > 1:
            assert (self.status[:, 1:] != self.status[:, :-1]).any()
        if full:
            deny_rows = [ri for ri, r in enumerate(self.rules) if is_deny(r)]
            for s in (PASS, FAIL, ERROR, SKIP, CPU, NOMATCH):
                assert (self.status[deny_rows] == s).any(), s
            for n in ARRAY_RULES:  # both ends of an undecided condition
                row = self.status[names.index(n)]
                arr = np.array([isinstance(x["spec"].get("zones"), list) for x in self.resources])
                assert (row[arr] == CPU).any() and (row[arr] != CPU).any(), n
            eb = self.status[names.index("error-beats-array")]
            arr = np.array([isinstance(x["spec"].get("zones"), list) for x in self.resources])
            assert (eb[arr] == ERROR).any()  # an unresolved string beside an array operand
            me = names.index("masked-error")
            noapp = np.array([x["kind"] == "Pod" and "app" not in (x["metadata"].get("labels") or {"app": 1})
                              for x in self.resources])
            assert noapp.any() and (self.status[me][noapp] == SKIP).all()  # SKIP wins over the error
