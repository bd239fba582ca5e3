"""A small independent restatement of the reference's validate.deny semantics
(pkg/engine/validation.go:299-339 validateDeny / getDenyMessage, variables/vars.go:76-80,315-366,
utils.go:392-406, variables/evaluate.go:42-78), the expected side of the deny tests next to the
golden cases (tests/golden/deny.json). Operators and the any / all fold come from
cond_model.Model; what differs from the preconditions is the resolver (an unresolved variable is an
error, and the whole conditions document is substituted before anything is evaluated) and the
verdict (true is FAIL, false is PASS)."""
from __future__ import annotations

import json
import re

import cond_model

UNKNOWN = cond_model.UNKNOWN
ERROR_PREFIX = "failed to substitute variables in deny conditions: "


class Unresolved(Exception):
    """gojmespath.NotFoundError, returned bare by substituteVariablesIfAny (vars.go:360-366)."""


class Model(cond_model.Model):
    def _query(self, var: str, resource):
        """As cond_model.Model._query, but a missing map key raises: `Unknown key "x" in path`."""
        assert var.startswith("request.object"), var
        cur, pos, rest = resource, 0, var[len("request.object"):]
        while pos < len(rest):
            m = self._STEP.match(rest, pos)
            assert m, var
            pos = m.end()
            if cur is None:
                continue
            if m.group(3) is not None:
                i = int(m.group(3))
                cur = cur[i] if isinstance(cur, list) and -len(cur) <= i < len(cur) else None
            else:
                k = m.group(1) if m.group(1) is not None else re.sub(r"\\(.)", r"\1", m.group(2))
                if not isinstance(cur, dict):
                    cur = None
                elif k not in cur:
                    raise Unresolved(f'Unknown key "{k}" in path')
                else:
                    cur = cur[k]
        return True, cur

    @staticmethod
    def conditions(block):
        """The conditions of an any / all block or the old list, in the traversal's canonical key
        order (all before any)."""
        if isinstance(block, list):
            return list(block)
        return list(block.get("all") or []) + list(block.get("any") or [])

    def errors(self, block, resource) -> list[str]:
        """The error of every distinct string of the block that does not resolve (SubstituteAll
        stops at the first it meets; which one that is depends on Go's map order)."""
        out, seen = [], set()
        for c in self.conditions(block):
            for side in ("key", "value"):
                s = c.get(side)
                if not isinstance(s, str) or s in seen:
                    continue
                seen.add(s)
                try:
                    self.substitute(s, resource)
                except Unresolved as e:
                    out.append(str(e))
        return out

    def deny(self, block, resource):
        """("error", [messages]) | ("fail" | "pass" | UNKNOWN, None)."""
        errs = self.errors(block, resource)
        if errs:
            return "error", [ERROR_PREFIX + e for e in errs]
        v = self.preconditions(block, resource)  # the same fold (EvaluateConditions)
        if v == UNKNOWN:
            return UNKNOWN, None
        return ("fail" if v else "pass"), None

    def message(self, rule: dict, resource, status: str) -> str:
        """getDenyMessage for "pass" / "fail"."""
        name = rule["name"]
        if status == "pass":
            return f"validation rule '{name}' passed."
        msg = (rule.get("validate") or {}).get("message") or ""
        if msg == "":
            return f"validation error: rule {name} failed"
        try:
            got = self.substitute(msg, resource)
        except Unresolved:
            return msg
        return got if isinstance(got, str) else json.dumps(got)
