"""validate.foreach entries with an `anyPattern` on the device (KV_COMPILE_FOREACH_ANYPATTERN),
without a GPU: the flag's value and its dependencies, rule routing under the flag combinations
(today's routing unchanged without the new flag), each scope limit, generated source and foreach
tables of policy sets without anyPattern entries (byte-identical with and without the flag), the
hand-derived cases of tests/golden/foreach_anypattern.json as device rules, the conditions on the
crafted data, and the crafted set through the sanitized host build of the lane body
kv_foreach_any_kernel runs (tools/kvemu/fepat.cpp) against the model of foreach_anypattern_data.py."""
import ctypes
import json
import os

import numpy as np
import pytest

import foreach_anypattern_data as fad
import foreach_pattern_data as fpd
from kyverno_amd import _native, batch, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SIZES = [1, 63, 65, 257]
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "foreach_anypattern.json")))
ALL = dict(foreach=True, foreach_pattern=True, foreach_entries=True, foreach_anypattern=True)


@pytest.fixture(scope="module")
def expected(orc):
    pol = fad.crafted_policy()
    return pol, {n: fad.Expected(orc, pol, fad.crafted_resources(n)) for n in EMU_SIZES + [513]}


# ------------------------------------------------------------------ flags and routes
def test_flag_value_and_dependencies():
    data = json.dumps([fad.crafted_policy()]).encode()
    h = ctypes.c_void_p()
    lib = _native.lib()
    F, P, E, A = batch.COMPILE_FOREACH, batch.COMPILE_FOREACH_PATTERN, batch.COMPILE_FOREACH_ENTRIES, \
        batch.COMPILE_FOREACH_ANYPATTERN
    assert A == 32
    for flags in (A, A | F, A | P, A | F | E, A | batch.COMPILE_SPECIALIZE):
        assert lib.kv_compile(data, len(data), flags, ctypes.byref(h), None) == -1, flags  # KV_E_INVALID
    with pytest.raises(_native.KvError):
        batch.PolicySet([fad.crafted_policy()], foreach=True, foreach_anypattern=True)
    for flags in (A | F | P, A | F | P | E):
        assert lib.kv_compile(data, len(data), flags, ctypes.byref(h), None) == 0, flags
        lib.kv_free_policyset(h)
    hdr = open(os.path.join(ROOT, "include", "kvgpu.h")).read()
    assert "KV_COMPILE_FOREACH_ANYPATTERN = 32" in hdr
    for s in ("kv_rule_foreach_anypattern", "kv_foreach_set_alternatives", "kv_result_foreach_alt",
              "kv_result_foreach_alt_error_message"):
        assert s in _native.EXPORTED_SYMBOLS and getattr(lib, s) is not None and s in hdr


def test_routes_under_the_flag_combinations():
    pol = fad.crafted_policy()
    rules = pol["spec"]["rules"]
    names = [r["name"] for r in rules]
    every = batch.PolicySet([pol], **ALL)
    for r, a in zip(rules, every.rules):
        if fad.on_device(r):
            assert (a.route, a.route_reason, a.foreach, a.foreach_pattern) == (batch.ROUTE_GPU, "", True, False), r["name"]
            assert a.foreach_anypattern == fad.n_alternatives(r), r["name"]
        else:
            assert (a.route, a.route_reason, a.foreach, a.foreach_anypattern) == (batch.ROUTE_CPU, "foreach", False, 0), \
                r["name"]
    assert every.rules[names.index("deny-then-any")].foreach_entries == 2
    # without the entries flag the chain stays routed, the single entries do not
    single = batch.PolicySet([pol], foreach=True, foreach_pattern=True, foreach_anypattern=True)
    for r, a in zip(rules, single.rules):
        on = fad.n_alternatives(r) > 0
        assert (a.route == batch.ROUTE_GPU, a.foreach_anypattern > 0) == (on, on), r["name"]
    # without the new flag: every rule of this set is routed, under every combination of the others
    for flags in ({}, dict(foreach=True), dict(foreach=True, foreach_pattern=True), dict(foreach=True, foreach_entries=True),
                  dict(foreach=True, foreach_pattern=True, foreach_entries=True)):
        ps = batch.PolicySet([pol], **flags)
        for a in ps.rules:
            assert (a.route, a.route_reason, a.foreach, a.foreach_anypattern) == (batch.ROUTE_CPU, "foreach", False, 0), \
                (flags, a.name)
        assert ps.foreach_info["sets"] == 0
    # an entry repeated in two rules (and behind rule preconditions) is one set; the chain's entry
    # shares the set of `three`
    sets = every.foreach_info["rule_sets"]
    assert sets[names.index("latest-or-c0")] == sets[names.index("shared")] == sets[names.index("behind-preconditions")] != 0
    lib = _native.lib()
    n = ctypes.c_uint32()
    for r, s in zip(rules, sets):
        if s:
            assert lib.kv_foreach_set_alternatives(every._h, s - 1, ctypes.byref(n)) == 0 and n.value == fad.n_alternatives(r)
    chain = every.foreach_chain_info["chain_sets"][0]
    assert lib.kv_foreach_set_alternatives(every._h, chain[0], ctypes.byref(n)) == 0 and n.value == 0
    assert chain[1] == sets[names.index("three")] - 1
    assert lib.kv_foreach_set_alternatives(every._h, 1000, ctypes.byref(n)) == -4  # KV_E_RANGE


def test_pattern_and_deny_sets_keep_their_routes_with_the_flag():
    """The pattern-entry set of foreach_pattern_data.py: the flag changes only its `entry-any-pattern` rule."""
    pol = fpd.crafted_policy()
    on = batch.PolicySet([pol], foreach=True, foreach_pattern=True, foreach_anypattern=True)
    off = batch.PolicySet([pol], foreach=True, foreach_pattern=True)
    for a, b in zip(on.rules, off.rules):
        if a.name == "entry-any-pattern":
            assert (a.route, a.foreach, a.foreach_pattern, a.foreach_anypattern) == (batch.ROUTE_GPU, True, False, 1)
            assert (b.route, b.route_reason) == (batch.ROUTE_CPU, "foreach")
        else:
            assert (a.route, a.route_reason, a.foreach, a.foreach_pattern) == (b.route, b.route_reason, b.foreach, b.foreach_pattern)
            assert a.foreach_anypattern == 0
    assert on.foreach_info["sets"] == off.foreach_info["sets"] + 1
    # the host fold leaves the any set's row unset and refuses it at the C boundary
    bt = batch.Batch(on, fpd.crafted_resources(5))
    st, el = on.foreach_fold(bt)
    row = on.foreach_info["rule_sets"][[r.name for r in on.rules].index("entry-any-pattern")] - 1
    assert (st[row] == 255).all()
    out = np.zeros(5, dtype=np.uint8)
    assert _native.lib().kv_batch_foreach_fold(on._h, bt._h, row, out.ctypes.data, None, 5) == -1


def _one(entry, **flags):
    pol = fpd.pd._policy("scope", [{"name": "r", "match": fad.POD, "validate": {"message": "m", "foreach": [entry]}}])
    ps = batch.PolicySet([pol], **(flags or ALL))
    r = ps.rules[0]
    return (r.route, r.route_reason, r.foreach_anypattern), ps


def test_each_scope_limit():
    GPU = lambda n: (batch.ROUTE_GPU, "", n)  # noqa: E731
    ROUTED = (batch.ROUTE_CPU, "foreach", 0)
    L = fad.LIST
    names = [{"name": f"c{j}"} for j in range(9)]
    assert _one({"list": L, "anyPattern": names[:1]})[0] == GPU(1)
    assert _one({"list": L, "anyPattern": names[:8]})[0] == GPU(8)
    got, ps = _one({"list": L, "anyPattern": names})
    assert got == ROUTED and ps.foreach_info["sets"] == 0 and ps.foreach_info["lists"] == 0  # (nothing left behind)
    assert _one({"list": L, "anyPattern": []})[0] == ROUTED
    assert _one({"list": L, "anyPattern": {"name": "c0"}})[0] == ROUTED
    assert _one({"list": L, "anyPattern": "c0"})[0] == ROUTED
    assert _one({"list": L, "anyPattern": [{"name": "c0"}, ["x"]]})[0] == ROUTED
    assert _one({"list": L, "anyPattern": [{"name": "c0"}], "pattern": {"name": "c0"}})[0] == ROUTED
    assert _one({"list": L, "anyPattern": [{"name": "c0"}], "context": []})[0] == ROUTED
    # each alternative within the limits of a pattern entry; a refusal at a later alternative leaves
    # nothing of the earlier ones
    for bad in ({"name": "{{element.name}}"}, {"(metadata)": {"name": "x"}}, {"spec": {"metadata": {"name": "x"}}}):
        got, ps = _one({"list": L, "anyPattern": [{"image": "a*"}, {"name": "c0"}, bad]})
        assert got == ROUTED, bad
        assert ps.foreach_info == {"sets": 0, "lists": 0, "conditions": 0, "strings": 0, "rule_sets": [0]}, bad
    # a $() reference anywhere in the list: the reference resolves it against the whole list, not
    # against the alternative (absolute, climbing above the alternative, or inside it)
    for ref in ("$(/image)", "$(../../../image)", "$(./../image)"):
        for alts in ([{"name": ref, "image": "x"}], [{"name": "c0"}, {"image": "x", "name": ref}], [{"a": {ref: "x"}}]):
            got, ps = _one({"list": L, "anyPattern": alts})
            assert got == ROUTED, (ref, alts)
            assert ps.foreach_info == {"sets": 0, "lists": 0, "conditions": 0, "strings": 0, "rule_sets": [0]}, (ref, alts)
    deep = {"a": "x"}
    for _ in range(15):
        deep = {"k": deep}
    assert _one({"list": L, "anyPattern": [{"name": "c0"}, deep]})[0] == ROUTED  # (more than 16 cursor levels)
    # a refused entry takes back the programs of its earlier alternatives: a policy set with the
    # refused rule in front compiles the rule behind it as if it stood alone
    good = {"name": "good", "match": fad.POD, "validate": {"foreach": [{"list": L, "anyPattern": [{"name": "c0"}]}]}}
    refused = {"name": "refused", "match": fad.POD, "validate": {"foreach": [
        {"list": L, "anyPattern": [{"image": "zz*"}, {"name": "{{element.name}}"}]}]}}
    alone = batch.PolicySet([fpd.pd._policy("p", [good])], **ALL)
    behind = batch.PolicySet([fpd.pd._policy("p", [refused, good])], **ALL)
    ress = fad.crafted_resources(7)
    assert alone.foreach_tables(batch.Batch(alone, ress)) == behind.foreach_tables(batch.Batch(behind, ress))


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


def test_sets_without_anypattern_entries_are_unchanged(tmp_path):
    """C2, the pattern twin and the chain twin: the flag changes no byte of the generated source or
    of the foreach tables."""
    ress = fad.crafted_resources(65)
    for name, pols, flags in (("c2", workloads.c2_policies(), dict(foreach=True, foreach_pattern=True)),
                              ("pattern", workloads.c2_foreach_pattern_policies(), dict(foreach=True, foreach_pattern=True)),
                              ("chain", workloads.c2_foreach_chain_policies(),
                               dict(foreach=True, foreach_pattern=True, foreach_entries=True))):
        a = _dump(pols, str(tmp_path), name + "-off.cpp", **flags)
        b = _dump(pols, str(tmp_path), name + "-on.cpp", foreach_anypattern=True, **flags)
        assert len(a) > 10000 and a == b, name
        pa, pb = batch.PolicySet(pols, **flags), batch.PolicySet(pols, foreach_anypattern=True, **flags)
        assert pa.foreach_tables(batch.Batch(pa, ress)) == pb.foreach_tables(batch.Batch(pb, ress)), name
        assert [(r.route, r.route_reason) for r in pa.rules] == [(r.route, r.route_reason) for r in pb.rules]


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_golden_cases_compile_to_device_rules(case):
    assert len(GOLDEN["cases"]) == 5 and case["origin"] == "derived"
    assert "no test of this form" in GOLDEN["description"]
    n = len(case["policy"]["spec"]["rules"][0]["validate"]["foreach"][0]["anyPattern"])
    r = batch.PolicySet([case["policy"]], foreach=True, foreach_pattern=True, foreach_anypattern=True).rules[0]
    assert (r.route, r.route_reason, r.foreach, r.foreach_anypattern) == (batch.ROUTE_GPU, "", True, n)
    r = batch.PolicySet([case["policy"]], foreach=True, foreach_pattern=True).rules[0]
    assert (r.route, r.route_reason) == (batch.ROUTE_CPU, "foreach")


def test_workload_twin():
    pols = workloads.c2_foreach_anypattern_policies()
    rules = pols[0]["spec"]["rules"]
    assert len(rules) == 100
    P = workloads.C2_FOREACH_PATTERNS
    for i in (0, 7, 8, 99):
        assert rules[i]["validate"]["foreach"][0]["anyPattern"] == [P[i % 8], P[(i + 1) % 8]]
    ps = batch.PolicySet(pols, foreach=True, foreach_pattern=True, foreach_anypattern=True)
    assert all(r.route == batch.ROUTE_GPU and r.foreach_anypattern == 2 for r in ps.rules)
    assert ps.foreach_info["sets"] == 8 and ps.foreach_info["lists"] == 1
    assert len(set(ps.foreach_info["rule_sets"])) == 8
    off = batch.PolicySet(pols, foreach=True, foreach_pattern=True)
    assert all((r.route, r.route_reason) == (batch.ROUTE_CPU, "foreach") for r in off.rules)


# ------------------------------------------------------------------ the data, the emulator
def test_check_honest(expected):
    for n, exp in expected[1].items():
        exp.check_honest(full=n == 513)


def test_message_forms_of_the_model(expected):
    """The three forms of buildAnyPatternErrorMessage and the unsubstituted message occur in the
    crafted set."""
    pol, exp = expected[0], expected[1][513]
    names = [r["name"] for r in pol["spec"]["rules"]]
    msgs = {names[ri]: m for (ri, k), m in exp.messages.items() if (ri, k) in exp.alts}
    head = "validation failed in foreach rule for validation error: "
    assert msgs["latest-or-c0"].startswith(head + "image of {{element.name}} is tagged latest. Rule latest-or-c0[0] failed at path ")
    assert msgs["three"].startswith(head + "one of three. Rule three[0] failed at path /image/. Rule three[1] ")
    assert msgs["cond-anchor"].startswith(head + "Rule cond-anchor[0] failed")
    assert any(": conditional anchor mismatch: " in m for (ri, k), m in exp.messages.items() if names[ri] == "cond-anchor")
    assert any(": global anchor mismatch: " in m for (ri, k), m in exp.messages.items() if names[ri] == "global-anchor")
    assert any(len(a) == 8 for a in exp.alts.values())


@pytest.mark.parametrize("n", EMU_SIZES)
def test_any_sets_on_the_emulator(expected, n):
    """The crafted set through the host build of the generated kernels; the driver fills the any
    sets' rows of the deny plane with kv_fe_any_lane, one lane at a time, under ASan / UBSan."""
    import kvemu_anypattern

    pol, exp = expected[0], expected[1][n]
    work = os.path.join(ROOT, "build", "kvemu_tests", f"foreach_anypattern_{n}")  # (a directory per case: workers run in parallel)
    exe = kvemu_anypattern.build([pol], work)
    st = kvemu_anypattern.run(exe, b"\n".join(json.dumps(r).encode() for r in exp.resources), work)
    bad = np.argwhere(st != exp.status)
    assert not len(bad), [(pol["spec"]["rules"][a]["name"], int(b), int(st[a, b]), int(exp.status[a, b])) for a, b in bad[:20]]


def test_int_typing_model_on_the_emulator(orc):
    """The guard counts for the alternatives the reference evaluates, those up to and including the
    first that passes. port-glob-first: on int ports every element is CPU. name-first: c0 passes at
    alternative 0 before the guarded one is reached, so a one-container Pod is PASS on int ports;
    the others reach it and are CPU. On 0.5-style values both rules are evaluated."""
    import kvemu_anypattern

    pol = fad.int_policy()
    work = os.path.join(ROOT, "build", "kvemu_tests", "foreach_anypattern_int")
    exe = kvemu_anypattern.build([pol], work)
    for fl in (False, True):
        ress = fad.crafted_resources(65, float_ports=fl)
        exp = fad.Expected(orc, pol, ress)
        st = kvemu_anypattern.run(exe, b"\n".join(json.dumps(r).encode() for r in ress), work)
        assert np.array_equal(st, exp.status), fl
        first = exp.status[0][exp.status[0] != fad.NOMATCH]
        second = exp.status[1][exp.status[1] != fad.NOMATCH]
        if fl:
            assert (first == fad.CPU).sum() * 5 < len(first) and (second == fad.CPU).sum() * 5 < len(second)
        else:
            assert set(first.tolist()) <= {fad.CPU, fad.SKIP}
            assert (second == fad.PASS).any() and (second == fad.CPU).any()
            one = [k for k, r in enumerate(ress) if isinstance(r["spec"].get("containers"), list)
                   and len(r["spec"]["containers"]) == 1 and r["kind"] == "Pod"
                   and isinstance(r["spec"]["containers"][0], dict) and None not in r["spec"]["containers"][0].values()]
            assert one and all(exp.status[1, k] == fad.PASS for k in one)
