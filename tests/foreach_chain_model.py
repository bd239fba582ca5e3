"""validate.foreach rules of several entries, restated from the reference
(pkg/engine/validation.go:204-283 validateForEach / addElementToContext, policyContext.go:47-60
Copy, context/context.go:74-86 AddJSON, :310-347 Checkpoint / Reset / Restore), on top of
foreach_model.py (one entry), which is imported and not changed. The expected side of the chain
tests next to tests/golden/foreach_chain.json. No Go toolchain is available: as its siblings, this
model is written from the Go source.

What this file adds:
 1. the entry loop: entries run in order; an entry whose list query fails (a missing map key) is
    `continue`d before any checkpoint; per element, in order, validate(); a SKIP is ignored, a PASS
    increments applyCount, which runs across the entries; the first other result ends the rule;
    after all entries PASS "rule passed" when applyCount > 0, else SKIP "rule skipped";
 2. the leak: PolicyContext.Copy() shares the JSONContext, and Reset() restores to the checkpoint
    without popping it, so after entry k's last element the raw context still holds `element` =
    that element merged over what entry k's checkpoint held, and entry k + 1's checkpoint copies
    that. With L_k the last element of entry k's list: B_1 = nothing; B_{k+1} = merge(B_k, L_k) when
    entry k had an element, B_k when its query failed or gave []. The `element` the variables of
    entry k see (entry preconditions, deny conditions, the message) is merge(B_k, e);
 3. the merge (jsonpatch.MergeMergePatches, restated from the upstream library's mergeDocs; the
    kyverno fork's source is not at hand, so parity here is unpinned): for documents without null,
    two maps merge key by key, recursively; any other value, arrays included, replaces;
 4. a `pattern` entry matches ctx.Element, the raw element (addElementToContext sets it from the
    element itself): the pattern walk does not see the leak, the entry's preconditions do.
Outside the device scope (CPU) as in foreach_model.py; an entry whose list is outside it makes the
rule CPU when the walk reaches it.
"""
from __future__ import annotations

import json

import cond_model
import foreach_model
import foreach_pattern_data as fpd

UNKNOWN = cond_model.UNKNOWN
HEAD, PASSED, SKIPPED = foreach_model.HEAD, foreach_model.PASSED, foreach_model.SKIPPED


def merge(base, over):
    """mergeDocs for documents without null: maps merge key by key, anything else replaces."""
    if not (isinstance(base, dict) and isinstance(over, dict)):
        return over
    out = dict(base)
    for k, v in over.items():
        out[k] = merge(out[k], v) if k in out else v
    return out


class Model(foreach_model.Model):
    def __init__(self, orc):
        super().__init__(orc)
        self.orc = orc
        self._memo = {}
        self.leak = True  # (False: every entry sees its raw element, for the tests' "what if" side)

    def pattern_element(self, rule, entry, resource, raw, seen):
        """validate() on one element of a pattern entry: the entry preconditions on the element as
        the variables see it (`seen`), MatchPattern on the raw element (foreach_pattern_data's
        oracle call, float typing); (code, detail)."""
        pre = entry.get("preconditions")
        if pre is not None:
            v = self.lenient.preconditions(pre, (resource, seen))
            if v == UNKNOWN:
                return "cpu", None
            if v is False:
                return "skip", None
        pat = entry["pattern"]
        if fpd.meets_int(self.orc, pat, raw):
            return "cpu", None
        key = (json.dumps(raw, sort_keys=True), json.dumps(pat, sort_keys=True))
        got = self._memo.get(key)
        if got is None:
            got = self._memo[key] = self.orc.match_pattern(json.dumps(raw), json.dumps(pat), res_mode=0)
        assert "panic" not in got, got
        if not got["set"]:
            return "pass", None
        if got["skip"]:
            return "skip", None
        return ("error" if got["path"] == "" else "fail"), got

    def pattern_message(self, rule, resource, seen, detail):
        """buildErrorMessage (validation.go:510-534), the message substituted in the element's context."""
        name, msg = rule["name"], rule["validate"].get("message", "")
        tail = f"failed at path {detail['path']}" if detail["path"] else f"execution error: {detail['msg']}"
        if not msg:
            return f"validation error: rule {name} {tail}"
        m = self.strict.message(rule, (resource, seen), "fail")
        return f"validation error: {m if m.endswith('.') else m + '.'} Rule {name} {tail}"

    def chain(self, rule: dict, resource):
        """(status, deciding entry | None, deciding element | None, [messages] | None, detail) of a
        rule of any number of entries, after match and the rule's own preconditions. `detail`: the
        oracle's pattern error of a deciding pattern entry, else None."""
        base = None  # B_k
        applied = 0
        for k, entry in enumerate(rule["validate"]["foreach"]):
            state, elems = self.elements(entry["list"], resource)
            if state == "cpu":
                return "cpu", k, None, None, None
            if state == "empty":
                continue  # (before any checkpoint: nothing changes)
            for i, raw in enumerate(elems):
                seen = raw if base is None else merge(base, raw)
                detail = None
                if "pattern" in entry:
                    c, detail = self.pattern_element(rule, entry, resource, raw, seen)
                    msgs = [HEAD + self.pattern_message(rule, resource, seen, detail)] if c in ("fail", "error") else None
                else:
                    c, msgs = self.element(rule, entry, resource, seen)
                if c == "skip":
                    continue
                if c == "pass":
                    applied += 1
                    continue
                return c, k, i, msgs, detail
            if elems and self.leak:
                base = elems[-1] if base is None else merge(base, elems[-1])
        return ("pass", None, None, [PASSED], None) if applied else ("skip", None, None, [SKIPPED], None)
