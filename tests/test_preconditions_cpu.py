"""Rule preconditions without a GPU (kvcond.cpp, kvblocks.h; reference pkg/engine/variables/operator/*.go,
evaluate.go:42-78, validation.go:175-193): the model and the library's host evaluator
(`kv_condition_eval`) against the reference's own test table (tests/golden/conditions.json), the
evaluator against the model on a seeded fuzz, rule routing, interning of condition sets, and the
specialized kernels with the gate on the host emulator (tests/kvemu.py)."""
import json
import os
import random

import numpy as np
import pytest

import cond_model
import precond_data as pd
from kyverno_amd import _native, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(orc):
    return cond_model.Model(orc)


# ------------------------------------------------------------------ fixtures as transcribed
def test_golden_fixture_shape():
    rows = pd.CONDITIONS["rows"]
    assert len(rows) == 263 and len(pd.ROWS) == 228
    assert sum(not r["in_scope"] for r in rows) == 35
    assert all(r["key_type"].startswith(("map", "[]")) for r in rows if not r["in_scope"])
    assert all(r["src"].startswith("pkg/engine/variables/evaluate_test.go:") for r in rows)
    # rows whose result depends on Go int being distinct from float64 (at most 5 may be so marked)
    assert sum(r["int_dependent"] is not None for r in rows) == 0
    assert len(pd.CONDITIONS["variable_cases"]) == 2
    assert len(pd.CLI_CASE["resources"]) == 2 and len(pd.CLI_CASE["results"]) == 2


# ------------------------------------------------------------------ model and evaluator pinned
@pytest.mark.parametrize("row", pd.ROWS, ids=lambda r: r["src"].split(":")[-1])
def test_model_matches_golden(model, row):
    assert model.evaluate(row["key"], row["operator"], row["value"]) == row["result"], row


@pytest.mark.parametrize("row", pd.ROWS, ids=lambda r: r["src"].split(":")[-1])
def test_condition_eval_matches_golden(row):
    got = batch.condition_eval({"key": row["key"], "operator": row["operator"], "value": row["value"]})
    assert got == row["result"], row


def test_condition_eval_out_of_scope_and_errors():
    import ctypes

    lib = _native.lib()
    out = ctypes.c_int(-1)
    KV_E_PARSE, KV_E_RANGE = -2, -4  # include/kvgpu.h
    scoped_out = [r for r in pd.CONDITIONS["rows"] if not r["in_scope"]]
    for c in scoped_out:  # map and slice keys
        raw = json.dumps({"key": c["key"], "operator": c["operator"], "value": c["value"]}).encode()
        assert lib.kv_condition_eval(raw, len(raw), ctypes.byref(out)) == KV_E_RANGE, c
    for raw in (b'{"key": 1, "operator": "DurationGreaterThan", "value": 2}',
                b'{"key": "a", "operator": "Equals", "value": {"a": 1}}'):
        assert lib.kv_condition_eval(raw, len(raw), ctypes.byref(out)) == KV_E_RANGE
    bad = b'{"key": 1, "operator": '
    assert lib.kv_condition_eval(bad, len(bad), ctypes.byref(out)) == KV_E_PARSE
    # operator names compare case-insensitively; an unknown one is false (evaluate.go:13-16)
    assert batch.condition_eval({"key": "a", "operator": "eQuAlS", "value": "a"}) is True
    assert batch.condition_eval({"key": "a", "operator": "Resembles", "value": "a"}) is False


def test_variable_cases(model):
    """Test_Eval_Equal_Var_Pass / _Fail: substituted under the preconditions resolver (Pass), or
    evaluated as written (Fail: the key stays the template text)."""
    for c in pd.CONDITIONS["variable_cases"]:
        key = model.substitute(c["key"], c["resource"]) if c["substitute"] else c["key"]
        assert model.evaluate(key, c["operator"], c["value"]) == c["result"], c["name"]
        assert batch.condition_eval({"key": key, "operator": c["operator"], "value": c["value"]}) == c["result"], c["name"]


def test_go_durations():
    ns = cond_model.parse_duration
    assert ns("1h") == 3600 * 10**9 and ns("60m") == ns("1h") and ns("1.5h") == 5400 * 10**9
    assert ns("0") == 0 and ns("-30s") == -30 * 10**9 and ns("1h30m") == 5400 * 10**9 and ns("100ms") == 10**8
    for bad in ("", "1", "h", "1d", "1 h", ".s", "3600", "+", "1h2"):
        assert ns(bad) is None, bad
    # parseDuration's "0" exclusion (operator.go:88-98): "0" alone is no duration
    assert batch.condition_eval({"key": "0", "operator": "Equals", "value": 0}) is False
    assert batch.condition_eval({"key": "0s", "operator": "Equals", "value": 0}) is True


# ------------------------------------------------------------------ fuzz against the model
STRS = ["", "a", "ab", "abc", "a*", "?b", "*", "a?c", "true", "<nil>"]
NUMS = [0, 1, 2, 10, -1, 1.5, 2.0, 0.5, 3600, 1024]
NUMSTRS = ["0", "1", "2", "10", "-1", "1.5", "2.0", "0.5", "1e1", "+2", "3600", " 1"]
DURS = ["1h", "60m", "30m", "5h", "2h", "0s", "1h30m", "3600s"]  # spellings of the golden rows and kin
QTYS = ["1Gi", "1024Mi", "10Gi", "100m", "1k", "1000", "0.1", "1Ki"]
JARRS = ['["a","b"]', '["1","2"]', "[]", "null", '[1]', '["a", null]', '["ab"', '[""]', '["1Gi"]']


def _scalar(rng):
    pool = rng.choice([STRS, NUMS, NUMSTRS, DURS, QTYS, [True, False], [None]])
    return rng.choice(pool)


def _operand(rng, is_key):
    k = rng.random()
    if is_key or k < 0.6:
        return _scalar(rng)
    if k < 0.8:
        return [_scalar(rng) for _ in range(rng.randrange(0, 4))]
    return rng.choice(JARRS)


OPS = ["Equals", "Equal", "NotEquals", "NotEqual", "In", "NotIn", "AnyIn", "AllIn", "AnyNotIn", "AllNotIn",
       "GreaterThan", "GreaterThanOrEquals", "LessThan", "LessThanOrEquals", "Resembles", "lessthan"]


def test_condition_eval_matches_model_fuzz(model):
    rng = random.Random(20260419)
    n, seen_true, bad = 6000, 0, []
    for _ in range(n):
        key, op, value = _operand(rng, True), rng.choice(OPS), _operand(rng, False)
        want = model.evaluate(key, op, value)       # (no case is skipped: the alphabet is in scope)
        got = batch.condition_eval({"key": key, "operator": op, "value": value})
        seen_true += want
        if got != want:
            bad.append((key, op, value, want, got))
    assert not bad, bad[:20]
    assert n // 10 < seen_true < n - n // 10  # both outcomes are exercised


# ------------------------------------------------------------------ routing
V = "{{request.object.metadata.labels.app}}"


def _cond(key=V, op="Equals", value="busybox"):
    return {"key": key, "operator": op, "value": value}


IN_SCOPE = {
    "old-list": [_cond()],
    "any": {"any": [_cond()]},
    "all": {"all": [_cond()]},
    "any-all": {"any": [_cond(), _cond(value="nginx")], "all": [_cond(op="NotEquals", value="x")]},
    "empty-list": [],
    "empty-map": {},
    "all-empty": {"all": []},
    "equal": {"all": [_cond(op="Equal")]},
    "notequals": {"all": [_cond(op="NotEquals")]},
    "notequal": {"all": [_cond(op="NotEqual")]},
    "in": {"all": [_cond(op="In", value=["a", "b"])]},
    "notin": {"all": [_cond(op="NotIn", value=["a", "b"])]},
    "anyin": {"all": [_cond(op="AnyIn", value=["a", 1, True, None])]},
    "allin": {"all": [_cond(op="AllIn", value='["a","b"]')]},
    "anynotin": {"all": [_cond(op="AnyNotIn", value=["a"])]},
    "allnotin": {"all": [_cond(op="AllNotIn", value="a")]},
    "gt": {"all": [_cond(op="GreaterThan", value=3)]},
    "ge": {"all": [_cond(op="GreaterThanOrEquals", value="1Gi")]},
    "lt": {"all": [_cond(op="LessThan", value="1h")]},
    "le": {"all": [_cond(op="LessThanOrEquals", value=2.5)]},
    "case-insensitive": {"all": [_cond(op="eQuALs")]},
    "unknown-operator": {"all": [_cond(op="Resembles")]},
    "variable-in-value": {"all": [_cond(key="busybox", value=V)]},
    "constant-folded": {"all": [_cond(key="a", value="a")], "any": [_cond(key=1, op="GreaterThan", value=0), _cond()]},
    "in-string": {"all": [_cond(key="x-" + V + "-{{request.object.metadata.namespace}}")]},
    "quoted-and-index": {"all": [_cond(key='{{request.object.metadata.labels."app.kubernetes.io/name"}}'),
                                 _cond(key="{{ request.object.spec.containers[0].image }}", value="nginx*")]},
    "null-operands": {"all": [_cond(value=None)]},
}
OUT_OF_SCOPE = {
    "request-operation": {"all": [_cond(key="{{request.operation}}", value="CREATE")]},
    "user-info": {"all": [_cond(key="{{request.userInfo.username}}")]},
    "at": {"all": [_cond(key="{{@}}")]},
    "custom-jmespath": {"all": [_cond(key="{{request.object.spec.containers[*].image}}")]},
    "both-sides": {"all": [_cond(value="{{request.object.metadata.name}}")]},
    "variable-in-list": {"all": [_cond(key="a", op="In", value=["x", V])]},
    "variable-in-map": {"all": [_cond(value={"a": V})]},
    "reference": {"all": [_cond(value="$(./../key)")]},
    "escape": {"all": [_cond(value="\\{{literal}}")]},
    "variable-in-operator": {"all": [_cond(op="{{request.object.metadata.name}}")]},
    "duration-operator": {"all": [_cond(op="DurationGreaterThan", value="1h")]},
    "map-operand": {"all": [_cond(value={"a": "b"})]},
    "list-key": {"all": [_cond(key=["a", "b"], op="AnyIn", value=V)]},
    "missing-key": {"all": [{"operator": "Equals", "value": "busybox"}]},
    "missing-value": {"all": [{"key": V, "operator": "Equals"}]},
    "any-empty": {"any": []},
    "unknown-field": {"all": [_cond()], "some": []},
    "not-a-block": "busybox",
}
PATTERN = {"message": "m", "pattern": {"spec": {"containers": [{"image": "*:*"}]}}}


def _routing_policy():
    rules = []
    for name, pre in list(IN_SCOPE.items()) + list(OUT_OF_SCOPE.items()):
        rules.append({"name": name, "match": pd.POD, "preconditions": pre, "validate": PATTERN})
    pre = {"all": [_cond()]}
    extra = [
        ("x-anypattern", True, {"message": "m", "anyPattern": [{"spec": {"hostNetwork": False}}, {"kind": "Pod"}]}, {}),
        ("x-pattern-variable", True, {"pattern": {"spec": {"serviceAccountName": "{{request.object.metadata.namespace}}"}}}, {}),
        ("x-constant-pattern", False, {"message": "m", "anyPattern": []}, {}),
        ("x-pattern-out-of-scope", False, {"pattern": {"metadata": {"name": "{{request.userInfo.username}}"}}}, {}),
        ("x-deny", False, {"deny": {"conditions": [_cond()]}}, {}),
    ]
    for name, _, validate, more in extra:
        rules.append({"name": name, "match": pd.POD, "preconditions": pre, "validate": validate, **more})
    rules.append({"name": "x-context", "match": pd.POD, "preconditions": pre, "validate": PATTERN,
                  "context": [{"name": "cm", "configMap": {"name": "a", "namespace": "b"}}]})
    rules.append({"name": "x-foreach", "match": pd.POD, "preconditions": pre,
                  "validate": {"foreach": [{"list": "request.object.spec.containers", "pattern": {"image": "*"}}]}})
    return pd._policy("routing", rules), {n: ok for n, ok, _, _ in extra}


def test_routing():
    """One rule per in-scope form (GPU route, no reason) and per out-of-scope form (CPU route, the
    reason callers already know); context and foreach keep their precedence."""
    pol, extra = _routing_policy()
    ps = batch.PolicySet([pol])
    got = {r.name: (r.route, r.route_reason) for r in ps.rules}
    for name in IN_SCOPE:
        assert got[name] == (batch.ROUTE_GPU, ""), (name, got[name])
    for name in OUT_OF_SCOPE:
        assert got[name] == (batch.ROUTE_CPU, "preconditions"), (name, got[name])
    for name, ok in extra.items():
        assert got[name] == ((batch.ROUTE_GPU, "") if ok else (batch.ROUTE_CPU, "preconditions")), (name, got[name])
    assert got["x-context"] == (batch.ROUTE_CPU, "context")
    assert got["x-foreach"] == (batch.ROUTE_CPU, "foreach")


def test_interning():
    """30 rules over 3 distinct precondition blocks compile to 3 condition sets (autogen triples
    every rule; real sets repeat one block across many rules)."""
    blocks = [{"all": [_cond()]},
              {"any": [_cond(value="a"), _cond(key="{{request.object.metadata.labels.tier}}", op="In", value=["x", "y"])]},
              [_cond(), _cond(key="{{request.object.metadata.labels.tier}}", op="NotEquals", value="z")]]
    rules = [{"name": f"r{i}", "match": pd.POD, "preconditions": json.loads(json.dumps(blocks[i % 3])), "validate": PATTERN}
             for i in range(30)]
    ps = batch.PolicySet([pd._policy("interning", rules)])
    assert all(r.route == batch.ROUTE_GPU for r in ps.rules)
    info = ps.precondition_info
    assert info == {"sets": 3, "conditions": 4, "strings": 2}, info
    # a policy set without preconditions has none
    assert batch.PolicySet([pd._policy("none", [{"name": "r", "match": pd.POD, "validate": PATTERN}])]).precondition_info["sets"] == 0


def test_exported_symbols():
    lib = _native.lib()
    for s in ("kv_result_precond_message", "kv_condition_eval", "kv_policyset_cond_sets"):
        assert s in _native.EXPORTED_SYMBOLS and getattr(lib, s) is not None
    hdr = open(os.path.join(ROOT, "include", "kvgpu.h")).read()
    assert "int kv_result_precond_message(const kv_result* r, uint32_t rule, uint64_t res, char* buf, size_t cap);" in hdr
    assert "int kv_condition_eval(const char* condition_json, size_t len, int* result);" in hdr


# ------------------------------------------------------------------ expected side, emulator
def test_crafted_expected_covers_the_cases(orc):
    """The crafted data holds what the GPU tests rely on: both ways an unknown condition ends
    (decided anyway, CPU), gated SKIPs next to conditional-anchor SKIPs, genuine FAILs."""
    pol, ress = pd.crafted_policy(), pd.crafted_resources(513)
    e = pd.Expected(orc, pol, ress)
    names = [r["name"] for r in pol["spec"]["rules"]]
    row = {n: i for i, n in enumerate(names)}
    arr = np.array([isinstance((r.get("spec") or {}).get("zones"), list) for r in ress])
    aa = row["any-all-array"]
    assert (e.status[aa][arr] == pd.CPU).any() and (e.status[aa][arr] != pd.CPU).any()
    assert ((e.status[aa] == pd.CPU) <= arr).all()
    ca = row["conditional-anchor"]
    assert (e.gated[ca]).any() and ((e.status[ca] == pd.SKIP) & ~e.gated[ca]).any()
    assert (e.status[row["unknown-operator"]][e.status[row["no-preconditions"]] != pd.NOMATCH] == pd.SKIP).all()
    assert np.array_equal(e.status[row["empty-list"]], e.status[row["no-preconditions"]])
    assert np.array_equal(e.status[row["empty-map"]], e.status[row["no-preconditions"]])
    for s in (pd.PASS, pd.FAIL, pd.SKIP, pd.NOMATCH, pd.CPU):
        assert (e.status == s).any(), s
    tiers = {json.dumps((r["metadata"].get("labels") or {}).get("tier")) for r in ress}
    assert len(tiers) >= 70


def test_specialized_kernels_on_the_emulator(orc):
    """The crafted set at 257 resources through the specialized kernels compiled for the host
    (tests/kvemu.py; the driver fills pre_st with the per-lane function the device kernel runs),
    against the decomposition."""
    import kvemu

    pol, ress = pd.crafted_policy(), pd.crafted_resources(257)
    e = pd.Expected(orc, pol, ress)
    work = os.path.join(ROOT, "build", "kvemu_tests", "preconditions")
    exe = kvemu.build([pol], work)
    st, _ = kvemu.run(exe, b"\n".join(json.dumps(r).encode() for r in ress), work)
    bad = np.argwhere(st != e.status)
    assert not len(bad), [(pol["spec"]["rules"][a]["name"], int(b), int(st[a, b]), int(e.status[a, b])) for a, b in bad[:20]]
