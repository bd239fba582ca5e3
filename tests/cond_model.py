"""A small independent restatement of the reference's precondition semantics for scalar keys
(pkg/engine/variables/operator/*.go, evaluate.go:42-78, vars.go:62-84, utils.go:445-458), used by
the precondition tests as the expected side next to the golden rows (tests/golden/conditions.json).

Operands are what encoding/json leaves in a kyverno.Condition: str, float / int (both float64),
bool, None, list. Globs and quantities come from the oracle bindings (orc.glob, orc.quantity,
orc.quantity_cmp); durations from a Go-duration parser below. `UNKNOWN` is the third truth value
of a condition whose variable is a map or array on the resource (outside the device scope)."""
from __future__ import annotations

import json
import math
import re

UNKNOWN = "unknown"


class OutOfScope(Exception):
    pass


_UNITS = {"ns": 1, "us": 1000, "µs": 1000, "μs": 1000, "ms": 10**6, "s": 10**9, "m": 60 * 10**9,
          "h": 3600 * 10**9}


def parse_duration(s: str):
    """time.ParseDuration -> nanoseconds or None: [-+]?([0-9]*(\\.[0-9]*)?[a-z]+)+, "0" is zero."""
    m = re.fullmatch(r"([-+]?)(.*)", s, re.S)
    neg, rest = m.group(1) == "-", m.group(2)
    if rest == "0":
        return 0
    if rest == "":
        return None
    total, pos = 0, 0
    tok = re.compile(r"(\d*)(?:\.(\d*))?([^\d.]+)")
    while pos < len(rest):
        t = tok.match(rest, pos)
        if not t or (t.group(1) == "" and not t.group(2)) or t.group(3) not in _UNITS:
            return None
        unit = _UNITS[t.group(3)]
        v = int(t.group(1) or "0")
        if v > 1 << 63 or v * unit > 1 << 63:
            return None
        v *= unit
        frac = t.group(2) or ""
        if frac.strip("0"):
            f, scale = int(frac[:18]), 10.0 ** len(frac[:18])
            v += int(float(f) * (float(unit) / scale))
        total += v
        if total > 1 << 63:
            return None
        pos = t.end()
    if not neg and total > (1 << 63) - 1:
        return None
    return -total if neg else total


def _seconds(ns: int) -> float:
    # Duration.Seconds(): d / Second truncates toward zero, d % Second keeps the sign
    sec = (abs(ns) // 10**9) * (-1 if ns < 0 else 1)
    nsec = ns - sec * 10**9
    return float(sec) + float(nsec) / 1e9


def parse_float(s: str):
    """strconv.ParseFloat(s, 64) for decimal spellings; None on error (out of range included)."""
    if re.fullmatch(r"[+-]?(inf|infinity)", s, re.I):
        return -math.inf if s[0] == "-" else math.inf
    if re.fullmatch(r"[+-]?nan", s, re.I):
        return math.nan
    if not re.fullmatch(r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?", s):
        return None
    f = float(s)
    return None if math.isinf(f) else f


def parse_int(s: str):
    if not re.fullmatch(r"[+-]?\d+", s):
        return None
    v = int(s)
    return v if -(1 << 63) <= v < (1 << 63) else None


def is_num(x) -> bool:
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def sprint(x) -> str:
    """fmt.Sprint of a decoded scalar (%v of a float64: shortest form, exponent from 1e21)."""
    if x is None:
        return "<nil>"
    if isinstance(x, bool):
        return "true" if x else "false"
    if is_num(x):
        f = float(x)
        if f == int(f) and abs(f) < 1e21:
            return str(int(f))
        return repr(f)
    if isinstance(x, str):
        return x
    raise OutOfScope(x)


class Model:
    def __init__(self, orc):
        self.orc = orc

    # -- helpers
    def _durations(self, key, value):
        """parseDuration (operator.go:80-139): seconds of both, or None."""
        kd = parse_duration(key) if isinstance(key, str) and key != "0" else None
        vd = parse_duration(value) if isinstance(value, str) and value != "0" else None
        if kd is None and vd is None:
            return None
        if kd is None:
            if not is_num(key):
                return None
            kd = int(key) * 10**9
        if vd is None:
            if not is_num(value):
                return None
            vd = int(value) * 10**9
        return _seconds(kd), _seconds(vd)

    def _glob(self, pattern: str, name: str) -> bool:
        return self.orc.glob(pattern, name)

    def _equal(self, key, value, ne: bool) -> bool:
        if isinstance(key, bool):
            return ne if not isinstance(value, bool) else (key == value) != ne
        if is_num(key):
            if is_num(value):
                return (float(value) == float(key)) != ne
            if isinstance(value, str):
                f = parse_float(value)
                return ne if f is None else (f == float(key)) != ne
            return ne
        if isinstance(key, str):
            d = self._durations(key, value)
            if d is not None:
                return (d[0] == d[1]) != ne
            if self.orc.quantity(key) is not None and isinstance(value, str):
                if self.orc.quantity(value) is None:
                    return False
                return (self.orc.quantity_cmp(key, value) == 0) != ne
            if isinstance(value, str):
                return self._glob(value, key) != ne
            return ne
        return False  # nil key: unsupported type in both handlers

    @staticmethod
    def _cmp(op: str, k: float, v: float) -> bool:
        return {"greaterthan": k > v, "greaterthanorequals": k >= v, "lessthan": k < v, "lessthanorequals": k <= v}[op]

    def _numeric_float(self, op, key: float, value) -> bool:
        if is_num(value):
            return self._cmp(op, key, float(value))
        if isinstance(value, str):
            d = self._durations(key, value)
            if d is not None:
                return self._cmp(op, *d)
            f = parse_float(value)
            if f is not None:
                return self._cmp(op, key, f)
            i = parse_int(value)
            return False if i is None else self._cmp(op, key, float(i))
        return False

    def _numeric(self, op, key, value) -> bool:
        if isinstance(key, bool) or key is None:
            return False
        if is_num(key):
            return self._numeric_float(op, float(key), value)
        d = self._durations(key, value)
        if d is not None:
            return self._cmp(op, *d)
        f = parse_float(key)
        if f is not None:
            return self._numeric_float(op, f, value)
        i = parse_int(key)
        if i is not None:
            return self._numeric_float(op, float(i), value)
        if self.orc.quantity(key) is not None:
            if not isinstance(value, str) or self.orc.quantity(value) is None:
                return False
            return self._cmp(op, float(self.orc.quantity_cmp(key, value)), 0.0)
        return False

    def _key_exists(self, key: str, value):
        """keyExistsInArray (in.go:58-94): True / False, None for an invalid type."""
        if isinstance(value, list):
            return any(self._glob(key, sprint(v)) for v in value)
        if isinstance(value, str):
            if self._glob(value, key):
                return True
            try:
                arr = json.loads(value)
            except ValueError:
                return None
            if arr is None:
                return False
            if not isinstance(arr, list) or not all(isinstance(x, str) or x is None for x in arr):
                return None
            return key in ["" if x is None else x for x in arr]
        return None

    # -- variables.Evaluate
    def evaluate(self, key, operator: str, value) -> bool:
        op = operator.lower()
        if isinstance(key, (dict, list)) or isinstance(value, dict) or op.startswith("duration"):
            raise OutOfScope((key, operator, value))
        if isinstance(value, list) and any(isinstance(x, (dict, list)) for x in value):
            raise OutOfScope(value)
        if op in ("equal", "equals"):
            return self._equal(key, value, False)
        if op in ("notequal", "notequals"):
            return self._equal(key, value, True)
        if op in ("greaterthan", "greaterthanorequals", "lessthan", "lessthanorequals"):
            return self._numeric(op, key, value)
        if op in ("in", "anyin", "allin", "notin", "anynotin", "allnotin"):
            if isinstance(key, bool) or key is None:
                return False
            e = self._key_exists(sprint(key), value)
            if e is None:
                return False
            return (not e) if "notin" in op else e
        return False  # unknown operator (evaluate.go:13-16)

    # -- SubstituteAllInPreconditions on one string (vars.go:62-84, 319-398), request.object paths
    _VAR = re.compile(r"^\{\{[^{}]*\}\}|[^\\]\{\{[^{}]*\}\}")
    _STEP = re.compile(r'\.([A-Za-z_][A-Za-z0-9_]*)|\."((?:[^"\\]|\\.)*)"|\[(-?\d+)\]')

    def _query(self, var: str, resource):
        """(found, value): a missing map key is an error (-> ""), a field of a non-map or an index of
        a non-array is null."""
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
                    return False, None
                else:
                    cur = cur[k]
        return True, cur

    def substitute(self, s, resource):
        """The operand after substitution: a typed value for a whole-string variable."""
        if not isinstance(s, str):
            return s
        value = s
        while True:
            vs = self._VAR.findall(value)
            if not vs:
                return value
            original = value
            for v in vs:
                old = v
                if not v.startswith("{{"):
                    v = v[1:]
                found, val = self._query(v.replace("{{", "").replace("}}", "").strip(), resource)
                if not found:
                    val = ""
                if original == v:
                    return val
                prefix = "" if old == v else old[0]
                text = val if isinstance(val, str) else json.dumps(val, separators=(",", ":"), sort_keys=True)
                value = original.replace(prefix + v, prefix + text, 1)

    def condition(self, cond: dict, resource):
        """True / False / UNKNOWN for one condition on one resource."""
        key, value = self.substitute(cond.get("key"), resource), self.substitute(cond.get("value"), resource)
        var_key = isinstance(cond.get("key"), str) and self._VAR.search(cond["key"])
        var_val = isinstance(cond.get("value"), str) and self._VAR.search(cond["value"])
        if (var_key and isinstance(key, (dict, list))) or (var_val and isinstance(value, (dict, list))):
            return UNKNOWN
        return self.evaluate(key, cond.get("operator", ""), value)

    def preconditions(self, pre, resource):
        """True / False / UNKNOWN of a preconditions block (old list form: AND): three-valued fold
        of evaluate.go:42-78."""
        if isinstance(pre, list):
            any_l, all_l = None, pre
        else:
            any_l, all_l = pre.get("any"), pre.get("all") or []
        def fold_any(cs):
            rs = [self.condition(c, resource) for c in cs]
            return True if True in rs else (UNKNOWN if UNKNOWN in rs else False)
        def fold_all(cs):
            rs = [self.condition(c, resource) for c in cs]
            return False if False in rs else (UNKNOWN if UNKNOWN in rs else True)
        a = True if any_l is None else fold_any(any_l)
        b = fold_all(all_l)
        if a is False or b is False:
            return False
        if a == UNKNOWN or b == UNKNOWN:
            return UNKNOWN
        return True
