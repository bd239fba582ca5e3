"""A small independent restatement of the reference's validate.foreach semantics
(pkg/engine/validation.go:108-115,156-283 validateForEach / newForeachValidator / validate,
utils.go:445-472 evaluateList, context/{context,evaluate}.go), the expected side of the foreach
tests next to the golden cases (tests/golden/foreach.json). No Go toolchain is available, so this
model is written from the Go source, as cond_model.py and deny_model.py are; operators, the any /
all fold and both resolvers come from them. What this file adds: the list query, the `element`
variable root, the order of the per-element steps and the reduction to one status.

Steps, per (rule, resource), for a rule of exactly one foreach entry:
 1. evaluateList(entry.list): a missing map key is NotFound, the entry contributes nothing; a result
    that is not a list is a one-element list;
 2. per element, in order: {"element": element} is merged into the context; the entry's
    preconditions run under the preconditions resolver (unresolved -> ""), not met is SKIP (ignored);
    the deny block runs under the strict resolver over the whole block first (unresolved -> ERROR),
    true is FAIL, false is PASS (applyCount++);
 3. the first element that is neither PASS nor SKIP ends the rule with its status and the message
    "validation failed in foreach rule for " + the element's message;
 4. else PASS "rule passed" when applyCount > 0, SKIP "rule skipped" otherwise.
Outside the device scope (CPU): a null list, a scalar or list element, a null anywhere inside an
element (the merge patch's treatment of nulls is pinned by no reference test), more than 2^16
elements, an operand that is a map or array.
"""
from __future__ import annotations

import cond_model
import deny_model

UNKNOWN = cond_model.UNKNOWN
HEAD = "validation failed in foreach rule for "
PASSED, SKIPPED = "rule passed", "rule skipped"
MAX_ELEMS = 1 << 16


class _ElementRoot:
    """`element<chain>` resolves against the element, everything else against request.object. The
    context is the pair (resource, element)."""

    def _query(self, var, ctx):
        resource, element = ctx
        if var == "element" or var.startswith(("element.", "element[")):
            return super()._query("request.object" + var[len("element"):], element)
        return super()._query(var, resource)


class Lenient(_ElementRoot, cond_model.Model):
    pass


class Strict(_ElementRoot, deny_model.Model):
    pass


def has_null(x) -> bool:
    if x is None:
        return True
    if isinstance(x, dict):
        return any(has_null(v) for v in x.values())
    if isinstance(x, list):
        return any(has_null(v) for v in x)
    return False


class Model:
    def __init__(self, orc):
        self.lenient, self.strict = Lenient(orc), Strict(orc)

    def elements(self, list_expr: str, resource):
        """("empty", []) | ("ok", [maps]) | ("cpu", None)."""
        try:
            _, got = deny_model.Model._query(self.strict, list_expr, resource)
        except deny_model.Unresolved:
            return "empty", []
        if isinstance(got, dict):
            got = [got]
        if not isinstance(got, list) or len(got) > MAX_ELEMS:
            return "cpu", None
        if any(not isinstance(e, dict) or has_null(e) for e in got):
            return "cpu", None
        return "ok", got

    def element(self, rule: dict, entry: dict, resource, element):
        """validate() on one element: ("skip" | "pass" | "fail" | "error" | "cpu", [messages])."""
        ctx = (resource, element)
        pre = entry.get("preconditions")
        if pre is not None:
            v = self.lenient.preconditions(pre, ctx)
            if v == UNKNOWN:
                return "cpu", None
            if v is False:
                return "skip", None
        v, errs = self.strict.deny(entry["deny"]["conditions"], ctx)
        if v == "error":
            return "error", [HEAD + e for e in errs]
        if v == UNKNOWN:
            return "cpu", None
        if v == "pass":
            return "pass", None
        return "fail", [HEAD + self.strict.message(rule, ctx, "fail")]

    def codes(self, rule: dict, resource):
        """The list state and the verdict of every element (no early exit)."""
        entry = rule["validate"]["foreach"][0]
        state, elems = self.elements(entry["list"], resource)
        if state != "ok":
            return state, []
        return state, [self.element(rule, entry, resource, e) for e in elems]

    def foreach(self, rule: dict, resource):
        """(status, deciding element index | None, [messages]) of the rule on the resource, after
        match and the rule's own preconditions."""
        state, codes = self.codes(rule, resource)
        if state == "cpu":
            return "cpu", None, None
        applied = 0
        for i, (c, msgs) in enumerate(codes):
            if c == "skip":
                continue
            if c == "pass":
                applied += 1
                continue
            return c, i, msgs
        return ("pass", None, [PASSED]) if applied else ("skip", None, [SKIPPED])
