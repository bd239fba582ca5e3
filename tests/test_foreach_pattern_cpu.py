"""validate.foreach entries with a `pattern` on the device (KV_COMPILE_FOREACH_PATTERN), without a
GPU: rule routing under the three flag combinations, the flag's dependency on KV_COMPILE_FOREACH,
the reference's own two pattern cases (tests/golden/foreach.json) as device rules, the generated
source of a policy set without pattern entries (the same text with and without the flag), the
conditions on the crafted data, and the crafted set through the sanitized host build of the walk
kv_foreach_pat_kernel runs (tools/kvemu/fepat.cpp) against the decomposition of
foreach_pattern_data.py."""
import ctypes
import json
import os

import numpy as np
import pytest

import foreach_data as fd
import foreach_pattern_data as fpd
from kyverno_amd import _native, batch, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SIZES = [1, 65, 257]
PATTERN_CASES = [c for c in fd.CASES if c["name"] in ("Test_foreach_container_pass", "Test_foreach_container_fail")]


@pytest.fixture(scope="module")
def expected(orc):
    pol = fpd.crafted_policy()
    return pol, {n: fpd.Expected(orc, pol, fpd.crafted_resources(n)) for n in EMU_SIZES + [513]}


# ------------------------------------------------------------------ flags and routes
def test_flag_needs_foreach():
    data = json.dumps([fpd.crafted_policy()]).encode()
    h = ctypes.c_void_p()
    lib = _native.lib()
    assert batch.COMPILE_FOREACH_PATTERN == 8
    assert lib.kv_compile(data, len(data), batch.COMPILE_FOREACH_PATTERN, ctypes.byref(h), None) == -1  # KV_E_INVALID
    assert lib.kv_compile(data, len(data), batch.COMPILE_FOREACH_PATTERN | batch.COMPILE_SPECIALIZE, ctypes.byref(h),
                          None) == -1
    with pytest.raises(_native.KvError):
        batch.PolicySet([fpd.crafted_policy()], foreach_pattern=True)
    hdr = open(os.path.join(ROOT, "include", "kvgpu.h")).read()
    assert "KV_COMPILE_FOREACH_PATTERN = 8" in hdr
    for s in ("kv_rule_foreach_pattern", "kv_result_foreach_path", "kv_result_foreach_error_message"):
        assert s in _native.EXPORTED_SYMBOLS and getattr(lib, s) is not None


def test_routes_under_the_three_flag_combinations():
    pol = fpd.crafted_policy()
    rules = pol["spec"]["rules"]
    both = batch.PolicySet([pol], foreach=True, foreach_pattern=True)
    one = batch.PolicySet([pol], foreach=True)
    none = batch.PolicySet([pol])
    for r, a, b, c in zip(rules, both.rules, one.rules, none.rules):
        if fpd.on_device(r):
            assert (a.route, a.route_reason, a.foreach, a.foreach_pattern) == (batch.ROUTE_GPU, "", True, True), r["name"]
        else:
            assert (a.route, a.route_reason, a.foreach, a.foreach_pattern) == (batch.ROUTE_CPU, "foreach", False, False), \
                r["name"]
        for x in (b, c):  # every rule of this set has a pattern entry (or is outside the scope anyway)
            assert (x.route, x.route_reason, x.foreach, x.foreach_pattern) == (batch.ROUTE_CPU, "foreach", False, False), \
                r["name"]
    # an entry repeated in two rules is one set; autogen-style copies would share it too
    sets = both.foreach_info["rule_sets"]
    names = [r["name"] for r in rules]
    assert sets[names.index("no-latest")] == sets[names.index("shared")] != 0
    assert both.foreach_info["sets"] == sum(fpd.on_device(r) for r in rules) - 2  # (behind-preconditions shares it too)
    assert both.foreach_info["lists"] == 3
    assert one.foreach_info["sets"] == 0 and none.foreach_info["sets"] == 0


def test_deny_entries_keep_their_sets_with_the_flag():
    """The deny-entry set of foreach_data.py: the flag changes only its `entry-pattern` rule."""
    pol = fd.crafted_policy()
    on = batch.PolicySet([pol], foreach=True, foreach_pattern=True)
    off = batch.PolicySet([pol], foreach=True)
    for r, a, b in zip(pol["spec"]["rules"], on.rules, off.rules):
        if r["name"] == "entry-pattern":
            assert (a.route, a.foreach, a.foreach_pattern) == (batch.ROUTE_GPU, True, True)
            assert (b.route, b.route_reason) == (batch.ROUTE_CPU, "foreach")
        else:
            assert (a.route, a.route_reason, a.foreach) == (b.route, b.route_reason, b.foreach) and not a.foreach_pattern
    assert on.foreach_info["sets"] == off.foreach_info["sets"] + 1
    # the host fold leaves the pattern set's row unset and refuses it at the C boundary
    b = batch.Batch(on, fd.crafted_resources(5))
    st, el = on.foreach_fold(b)
    ps_row = on.foreach_info["rule_sets"][[r["name"] for r in pol["spec"]["rules"]].index("entry-pattern")] - 1
    assert (st[ps_row] == 255).all() and (st[np.arange(len(st)) != ps_row] != 255).all()
    out = np.zeros(5, dtype=np.uint8)
    assert _native.lib().kv_batch_foreach_fold(on._h, b._h, ps_row, out.ctypes.data, None, 5) == -1


@pytest.mark.parametrize("case", PATTERN_CASES, ids=lambda c: c["name"])
def test_reference_cases_compile_to_device_rules(case):
    assert len(PATTERN_CASES) == 2
    r = batch.PolicySet([case["policy"]], foreach=True, foreach_pattern=True).rules[0]
    assert (r.route, r.route_reason, r.foreach, r.foreach_pattern) == (batch.ROUTE_GPU, "", True, True)
    r = batch.PolicySet([case["policy"]], foreach=True).rules[0]
    assert (r.route, r.route_reason) == (batch.ROUTE_CPU, "foreach")


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


def test_generated_source_without_pattern_entries_is_unchanged(tmp_path):
    """Policy sets without pattern entries: the flag changes no byte of the generated source."""
    for name, pols in (("c2", workloads.c2_policies()), ("c2-foreach", workloads.c2_foreach_policies())):
        a = _dump(pols, str(tmp_path), name + "-off.cpp", foreach=True)
        b = _dump(pols, str(tmp_path), name + "-on.cpp", foreach=True, foreach_pattern=True)
        assert len(a) > 10000 and a == b, name


def test_workload_twin():
    pols = workloads.c2_foreach_pattern_policies()
    assert len(pols[0]["spec"]["rules"]) == 100
    ps = batch.PolicySet(pols, foreach=True, foreach_pattern=True)
    assert all(r.route == batch.ROUTE_GPU and r.foreach_pattern for r in ps.rules)
    assert ps.foreach_info["sets"] == 8 and ps.foreach_info["lists"] == 1
    assert all((r.route, r.route_reason) == (batch.ROUTE_CPU, "foreach") for r in batch.PolicySet(pols, foreach=True).rules)


# ------------------------------------------------------------------ the data, the emulator
def test_check_honest(expected):
    for n, exp in expected[1].items():
        exp.check_honest(full=n == 513)


def test_int_typing_model(orc):
    s = lambda p: fpd.sensitive(orc, p)  # noqa: E731
    assert not any(s(p) for p in (80, True, None, "*", ">1000", "<1024", "80", "1Gi", "100-200", ">=1 & <=5", "10|20"))
    assert all(s(p) for p in ("?0", "8*", "!80?", "80|8?", "ok", "?*"))
    assert fpd.meets_int(orc, {"port": "?0"}, {"port": 80}) and not fpd.meets_int(orc, {"port": "?0"}, {"port": 0.5})
    assert not fpd.meets_int(orc, {"port": "<1024"}, {"port": 80})
    assert fpd.meets_int(orc, {"port": 80}, {"port": 1 << 53}) and not fpd.meets_int(orc, {"port": 80}, {"port": (1 << 53) - 1})
    assert fpd.meets_int(orc, {"=(ports)": [{"containerPort": "8*"}]}, {"ports": [{"containerPort": 8443}]})


@pytest.mark.parametrize("n", EMU_SIZES)
def test_walk_on_the_emulator(expected, n):
    """The crafted set through the host build of the generated kernels; the driver fills the pattern
    sets' rows of the deny plane with the walk of kvwalk.h, one lane at a time, under ASan / UBSan."""
    import kvemu_pattern

    pol, exp = expected[0], expected[1][n]
    work = os.path.join(ROOT, "build", "kvemu_tests", f"foreach_pattern_{n}")  # (a directory per case: workers run in parallel)
    exe = kvemu_pattern.build([pol], work)
    st = kvemu_pattern.run(exe, b"\n".join(json.dumps(r).encode() for r in exp.resources), work)
    bad = np.argwhere(st != exp.status)
    assert not len(bad), [(pol["spec"]["rules"][a]["name"], int(b), int(st[a, b]), int(exp.status[a, b])) for a, b in bad[:20]]


def test_int_set_on_the_emulator(orc):
    """{"port": "?0"}: on int ports every matched pair with elements is CPU; on 0.5-style values the
    pattern is evaluated."""
    import kvemu_pattern

    pol = fpd.int_policy()
    work = os.path.join(ROOT, "build", "kvemu_tests", "foreach_pattern_int")
    exe = kvemu_pattern.build([pol], work)
    for fl in (False, True):
        ress = fpd.crafted_resources(65, float_ports=fl)
        exp = fpd.Expected(orc, pol, ress)
        st = kvemu_pattern.run(exe, b"\n".join(json.dumps(r).encode() for r in ress), work)
        assert np.array_equal(st, exp.status), fl
        row = exp.status[0][exp.status[0] != fpd.NOMATCH]
        if fl:
            assert (row == fpd.FAIL).any() and (row == fpd.CPU).sum() * 5 < len(row)
        else:
            assert set(row.tolist()) <= {fpd.CPU, fpd.SKIP}


def test_typing_arms_on_the_emulator(orc):
    """The other arms of the int-typing guard through the host build of the walk: |n| >= 2^53 under a
    number pattern (2^53 - 1 is evaluated), an int inside a nested list under a glob, ints in a
    scalar list (the leaf that walks every element)."""
    import kvemu_pattern

    pol, ress = fpd.typing_policy(), fpd.typing_resources()
    exp = fpd.Expected(orc, pol, ress)
    C, F, P = fpd.CPU, fpd.FAIL, fpd.PASS
    assert exp.status[0, 1:4].tolist() == [C, F, C] and exp.status[1, 4:7].tolist() == [C, P, F]
    assert exp.status[2, 7:10].tolist() == [P, C, F] and exp.status[3, 7:12].tolist() == [C, C, P, C, P]
    work = os.path.join(ROOT, "build", "kvemu_tests", "foreach_pattern_typing")
    exe = kvemu_pattern.build([pol], work)
    st = kvemu_pattern.run(exe, b"\n".join(json.dumps(r).encode() for r in ress), work)
    assert np.array_equal(st, exp.status), (st.tolist(), exp.status.tolist())


def test_rule_name_with_an_anchor_phrase_is_routed_in_either_order():
    """A rule whose name holds an anchor-error phrase stays on the CPU whether its (list, pattern) set
    was interned by an earlier rule or not."""
    a = fpd._rule("plain", {"image": "!*:latest"})
    b = fpd._rule("conditional anchor mismatch", {"image": "!*:latest"})
    for rules in ([a, b], [b, a]):
        ps = batch.PolicySet([fpd.pd._policy("magic", rules)], foreach=True, foreach_pattern=True)
        got = {r.name: (r.route, r.route_reason, r.foreach_pattern) for r in ps.rules}
        assert got["plain"] == (batch.ROUTE_GPU, "", True)
        assert got["conditional anchor mismatch"] == (batch.ROUTE_CPU, "foreach", False)
