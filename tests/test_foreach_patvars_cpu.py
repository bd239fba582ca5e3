"""`{{element...}}` / `{{request.object...}}` variables in the patterns of validate.foreach entries on
the device (KV_COMPILE_FOREACH_PATVARS), without a GPU: the flag's value and its dependencies, the
reference's own test as a device rule (routed without the flag), each out-of-scope form, policy
sets without such entries (byte-identical generated source and foreach tables with and without the
flag), the conditions on the crafted data, the crafted set through the sanitized host build of the
lane bodies kv_foreach_patv_kernel / kv_foreach_anyv_kernel run (tools/kvemu/fepat.cpp) against the
model of foreach_patvars_data.py, and the host twin of kv_fe_subst on every outcome order."""
import ctypes
import json
import os

import numpy as np
import pytest

import foreach_pattern_data as fpd
import foreach_patvars_data as fvd
from kyverno_amd import _native, batch, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SIZES = [1, 65]
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "foreach_patvars.json")))
ALL = fvd.ALL


@pytest.fixture(scope="module")
def expected(orc):
    pol = fvd.crafted_policy()
    return pol, {n: fvd.Expected(orc, pol, fvd.crafted_resources(n)) for n in EMU_SIZES + [63]}


# ------------------------------------------------------------------ flags and routes
def test_flag_value_and_dependencies():
    data = json.dumps([fvd.crafted_policy()]).encode()
    h = ctypes.c_void_p()
    lib = _native.lib()
    F, P, E, A, V = batch.COMPILE_FOREACH, batch.COMPILE_FOREACH_PATTERN, batch.COMPILE_FOREACH_ENTRIES, \
        batch.COMPILE_FOREACH_ANYPATTERN, batch.COMPILE_FOREACH_PATVARS
    assert V == 64
    for flags in (V, V | F, V | P, V | F | E, V | F | A, V | batch.COMPILE_SPECIALIZE):
        assert lib.kv_compile(data, len(data), flags, ctypes.byref(h), None) == -1, flags  # KV_E_INVALID
    with pytest.raises(_native.KvError):
        batch.PolicySet([fvd.crafted_policy()], foreach=True, foreach_patvars=True)
    for flags in (V | F | P, V | F | P | E, V | F | P | A, V | F | P | E | A):
        assert lib.kv_compile(data, len(data), flags, ctypes.byref(h), None) == 0, flags
        lib.kv_free_policyset(h)
    hdr = open(os.path.join(ROOT, "include", "kvgpu.h")).read()
    assert "KV_COMPILE_FOREACH_PATVARS = 64" in hdr
    for s in ("kv_rule_foreach_patvars", "kv_result_foreach_subst_error", "kv_batch_foreach_subst"):
        assert s in _native.EXPORTED_SYMBOLS and getattr(lib, s) is not None and s in hdr


def test_reference_fixture_is_a_device_rule_with_the_flag():
    """Test_foreach_element_validation: (ROUTE_GPU, "") with the flag, (ROUTE_CPU, "foreach") without."""
    assert GOLDEN["src"].startswith("pkg/engine/validation_test.go:2846-2892")
    case = GOLDEN["cases"][0]
    assert case["policy"]["spec"]["rules"][0]["validate"]["foreach"][0]["pattern"] == {"name": "{{ element.name }}"}
    r = batch.PolicySet([case["policy"]], foreach=True, foreach_pattern=True, foreach_patvars=True).rules[0]
    assert (r.route, r.route_reason, r.foreach, r.foreach_pattern, r.foreach_patvars) == (batch.ROUTE_GPU, "", True, True, True)
    for flags in ({}, dict(foreach=True), dict(foreach=True, foreach_pattern=True),
                  dict(foreach=True, foreach_pattern=True, foreach_entries=True, foreach_anypattern=True)):
        r = batch.PolicySet([case["policy"]], **flags).rules[0]
        assert (r.route, r.route_reason, r.foreach, r.foreach_patvars) == (batch.ROUTE_CPU, "foreach", False, False), flags


def test_reference_fixture_on_the_emulator():
    import kvemu_patvars

    case = GOLDEN["cases"][0]
    work = os.path.join(ROOT, "build", "kvemu_tests", "foreach_patvars_fixture")
    exe = kvemu_patvars.build([case["policy"]], work)
    st = kvemu_patvars.run(exe, json.dumps(case["resource"]).encode(), work)
    assert st.shape == (1, 1) and batch.STATUS_NAMES[int(st[0, 0])] == case["status"] == "pass"


def test_routes_of_the_crafted_set():
    pol = fvd.crafted_policy()
    rules = pol["spec"]["rules"]
    every = batch.PolicySet([pol], **ALL)
    for r, a in zip(rules, every.rules):
        if fvd.on_device(r):
            assert (a.route, a.route_reason, a.foreach) == (batch.ROUTE_GPU, "", True), r["name"]
            assert a.foreach_patvars == fvd.rule_has_variables(r), r["name"]
        else:
            assert (a.route, a.route_reason, a.foreach, a.foreach_patvars) == (batch.ROUTE_CPU, "foreach", False, False), r["name"]
    # an entry repeated in two rules is one set
    names = [r["name"] for r in rules]
    sets = every.foreach_info["rule_sets"]
    assert sets[names.index("name-is-alias")] == sets[names.index("shared")] == sets[names.index("behind-preconditions")] != 0
    # without the new flag: the rules with variables are routed, the one without is not
    off = batch.PolicySet([pol], foreach=True, foreach_pattern=True, foreach_entries=True, foreach_anypattern=True)
    for r, a in zip(rules, off.rules):
        on = fvd.on_device(r) and not fvd.rule_has_variables(r)
        assert (a.route == batch.ROUTE_GPU, a.route_reason) == (on, "" if on else "foreach"), r["name"]
        assert not a.foreach_patvars
    assert off.foreach_info["sets"] == 1 and off.foreach_info["strings"] == 0


def _one(pattern, key="pattern", **flags):
    entry = {"list": fvd.LIST, key: pattern}
    pol = fpd.pd._policy("scope", [{"name": "r", "match": fvd.POD, "validate": {"message": "m", "foreach": [entry]}}])
    ps = batch.PolicySet([pol], **(flags or ALL))
    r = ps.rules[0]
    return (r.route, r.route_reason, r.foreach_patvars), ps


def test_each_scope_limit():
    GPU = (batch.ROUTE_GPU, "", True)
    ROUTED = (batch.ROUTE_CPU, "foreach", False)
    NOTHING = {"sets": 0, "lists": 0, "conditions": 0, "strings": 0, "rule_sets": [0]}
    for good in ({"name": "{{element.name}}"}, {"name": "{{ element.name }}"}, {"name": "x-{{element.a.b}}-{{element.c[0]}}"},
                 {"name": '{{element."a.b"}}'}, {"name": "{{request.object.metadata.namespace}}"},
                 {"name": "{{request.object.metadata.name}}/{{element.name}}"}, {"=(a)": [{"b": "{{element.b}}"}]},
                 {"args": ["{{element.arg0}}"]}):
        assert _one(good)[0] == GPU, good
    for bad in ({"{{element.name}}": "x"}, {"name": "{{element}}"}, {"name": "{{@}}"}, {"name": "{{ to_upper(element.name) }}"},
                {"name": "{{ element.{{request.object.metadata.name}} }}"}, {"name": "{{element.a}}", "image": "\\{{element.b}}"},
                {"image": "{{element.alias}}", "name": "$(./../image)"}, {"metadata": {"name": "{{element.name}}"}},
                {"name": "{{serviceAccountName}}"}, {"name": "{{request.operation}}"}, {"name": "{{element.a | length(@)}}"}):
        got, ps = _one(bad)
        assert got == ROUTED, bad
        assert ps.foreach_info == NOTHING, bad  # (nothing left behind)
    assert _one([{"name": "c0"}, {"name": "{{element.name}}"}], key="anyPattern")[0] == GPU
    got, ps = _one([{"name": "{{element.name}}"}, {"{{element.name}}": "x"}], key="anyPattern")
    assert got == ROUTED and ps.foreach_info == NOTHING
    # a refused rule in front leaves nothing that changes the rule behind it
    good = {"name": "good", "match": fvd.POD, "validate": {"foreach": [{"list": fvd.LIST, "pattern": {"name": "{{element.alias}}"}}]}}
    refused = {"name": "refused", "match": fvd.POD, "validate": {"foreach": [
        {"list": fvd.LIST, "anyPattern": [{"image": "{{element.image}}"}, {"name": "{{element}}"}]}]}}
    alone = batch.PolicySet([fpd.pd._policy("p", [good])], **ALL)
    behind = batch.PolicySet([fpd.pd._policy("p", [refused, good])], **ALL)
    ress = fvd.crafted_resources(7)
    assert alone.foreach_tables(batch.Batch(alone, ress)) == behind.foreach_tables(batch.Batch(behind, ress))


def test_a_deny_string_of_the_same_list_shares_the_row():
    deny = {"name": "d", "match": fvd.POD, "validate": {"foreach": [{"list": fvd.LIST, "deny": {"conditions": {"all": [
        {"key": "{{element.alias}}", "operator": "Equals", "value": "x"}]}}}]}}
    pat = {"name": "p", "match": fvd.POD, "validate": {"foreach": [{"list": fvd.LIST, "pattern": {"name": "{{element.alias}}"}}]}}
    other = {"name": "q", "match": fvd.POD, "validate": {"foreach": [{"list": fvd.LIST, "pattern": {"name": "{{element.other}}"}}]}}
    assert batch.PolicySet([fpd.pd._policy("p", [deny, pat])], **ALL).foreach_info["strings"] == 1
    assert batch.PolicySet([fpd.pd._policy("p", [deny, pat, other])], **ALL).foreach_info["strings"] == 2


def _dump(pols, tmp, name, **flags):
    path = os.path.join(tmp, name)
    old = {k: os.environ.get(k) for k in ("KVGPU_JIT_DUMP", "KVGPU_JIT_SKIP_COMPILE")}
    os.environ.update(KVGPU_JIT_DUMP=path, KVGPU_JIT_SKIP_COMPILE="1")
    try:
        batch.PolicySet(pols, specialize=True, **flags)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return open(path, "rb").read()


def test_sets_without_pattern_variables_are_unchanged(tmp_path):
    """C2, the pattern twin, the any twin and the chain twin: the flag changes no byte of the generated
    source or of the foreach tables, and no route."""
    ress = fvd.crafted_resources(65)
    base = dict(foreach=True, foreach_pattern=True)
    for name, pols, flags in (("c2", workloads.c2_policies(), base),
                              ("pattern", workloads.c2_foreach_pattern_policies(), base),
                              ("any", workloads.c2_foreach_anypattern_policies(), dict(base, foreach_anypattern=True)),
                              ("chain", workloads.c2_foreach_chain_policies(), dict(base, foreach_entries=True))):
        a = _dump(pols, str(tmp_path), name + "-off.cpp", **flags)
        b = _dump(pols, str(tmp_path), name + "-on.cpp", foreach_patvars=True, **flags)
        assert len(a) > 10000 and a == b, name
        pa, pb = batch.PolicySet(pols, **flags), batch.PolicySet(pols, foreach_patvars=True, **flags)
        assert pa.foreach_tables(batch.Batch(pa, ress)) == pb.foreach_tables(batch.Batch(pb, ress)), name
        assert [(r.route, r.route_reason) for r in pa.rules] == [(r.route, r.route_reason) for r in pb.rules]
        assert not any(r.foreach_patvars for r in pb.rules)


def test_workload_twin():
    pols = workloads.c2_foreach_patvars_policies()
    rules = pols[0]["spec"]["rules"]
    assert len(rules) == 100
    text = json.dumps(pols)
    assert "{{element.name}}" in text and "{{request.object.metadata.namespace}}" in text
    ps = batch.PolicySet(pols, foreach=True, foreach_pattern=True, foreach_patvars=True)
    assert all(r.route == batch.ROUTE_GPU and r.foreach_pattern for r in ps.rules)
    assert any(r.foreach_patvars for r in ps.rules) and not all(r.foreach_patvars for r in ps.rules)
    assert ps.foreach_info["sets"] == len(workloads.C2_FOREACH_PATVARS_PATTERNS) and ps.foreach_info["lists"] == 1
    off = batch.PolicySet(pols, foreach=True, foreach_pattern=True)
    for r, a in zip(ps.rules, off.rules):
        assert (a.route == batch.ROUTE_GPU) == (not r.foreach_patvars), r.name


# ------------------------------------------------------------------ the data, the emulator
def test_check_honest(expected):
    for n, exp in expected[1].items():
        exp.check_honest()


@pytest.mark.parametrize("n", EMU_SIZES)
def test_crafted_set_on_the_emulator(expected, n):
    """The crafted set through the host build of the generated kernels; the driver fills the rows of
    the sets with variable strings with kv_fe_pat_lane<true> / kv_fe_any_lane<true>, one lane at a
    time, under ASan / UBSan."""
    import kvemu_patvars

    pol, exp = expected[0], expected[1][n]
    work = os.path.join(ROOT, "build", "kvemu_tests", f"foreach_patvars_{n}")  # (a directory per case: workers run in parallel)
    exe = kvemu_patvars.build([pol], work)
    st = kvemu_patvars.run(exe, b"\n".join(json.dumps(r).encode() for r in exp.resources), work)
    bad = np.argwhere(st != exp.status)
    assert not len(bad), [(pol["spec"]["rules"][a]["name"], int(b), int(st[a, b]), int(exp.status[a, b])) for a, b in bad[:20]]


def test_int_typing_is_decided_per_substituted_value(orc):
    """A substituted glob ("?0") over an int-typed port is CPU; over a float port it is evaluated."""
    import kvemu_patvars

    pol = fvd.int_policy()
    work = os.path.join(ROOT, "build", "kvemu_tests", "foreach_patvars_int")
    exe = kvemu_patvars.build([pol], work)
    for fl in (False, True):
        ress = fvd.crafted_resources(65, float_ports=fl)
        exp = fvd.Expected(orc, pol, ress)
        st = kvemu_patvars.run(exe, b"\n".join(json.dumps(r).encode() for r in ress), work)
        assert np.array_equal(st, exp.status), fl
        first = exp.status[0][exp.status[0] != fvd.NOMATCH]
        if fl:
            assert (first == fvd.CPU).sum() * 5 < len(first) and (first == fvd.FAIL).any()
        else:
            assert set(first.tolist()) <= {fvd.CPU, fvd.SKIP}
        second = exp.status[1][exp.status[1] != fvd.NOMATCH]
        assert (second == fvd.PASS).any()


# ------------------------------------------------------------------ kv_fe_subst on the host
ORDER_CASES = [
    # (pattern, element, expected code): `a` comes before `b` in traversal order
    ("E before C", {"a": "{{element.a}}", "b": "x-{{element.b}}"}, {"b": "{{ to_upper('x') }}"}, fvd.ERROR),
    ("C before E", {"a": "x-{{element.b}}", "b": "{{element.a}}"}, {"b": "{{ to_upper('x') }}"}, fvd.CPU),
    ("M then E", {"a": "{{element.a}}", "b": "x-{{element.b}}"}, {"a": {"k": 1}}, fvd.ERROR),
    ("M alone", {"a": "{{element.a}}", "b": "x-{{element.b}}"}, {"a": [1, 2], "b": "y"}, fvd.CPU),
    ("E then M", {"a": "{{element.a}}", "b": "{{element.b}}"}, {"b": {"k": 1}}, fvd.ERROR),
    ("all leaves", {"a": "{{element.a}}", "b": "x-{{element.b}}"}, {"a": 1.5, "b": "y"}, 0),
]


@pytest.mark.parametrize("name,pattern,element,want", ORDER_CASES, ids=[c[0] for c in ORDER_CASES])
def test_subst_verdict_on_the_host(orc, name, pattern, element, want):
    """kv_fe_subst's host twin (kv_batch_foreach_subst) against the model, which asks the oracle: the
    first error or out-of-scope outcome in traversal order decides, otherwise a map or an array in a
    leaf's place is CPU."""
    pol = fpd.pd._policy("order", [fvd._rule("r", pattern)])
    other = {"name": "c1", "a": "s", "b": "t"}
    res = {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "p", "namespace": "ns"},
           "spec": {"containers": [other, element]}}
    kind, val = fvd.Model(orc).substitute(pattern, res, element)
    assert {"doc": 0, "error": fvd.ERROR, "cpu": fvd.CPU}[kind] == want, (kind, val)
    ps = batch.PolicySet([pol], foreach=True, foreach_pattern=True, foreach_patvars=True)
    assert ps.rules[0].foreach_patvars
    b = batch.Batch(ps, [res])
    code, text = ps.foreach_subst(b, 0, 0, 1)
    assert code == want
    assert text == (val if kind == "error" else None)
    assert ps.foreach_subst(b, 0, 0, 0) == (0, None)
    with pytest.raises(RuntimeError):
        ps.foreach_subst(b, 0, 0, 2)  # (KV_E_RANGE: the list has two elements)
