"""validate.foreach entries with a `pattern` on the device (KV_COMPILE_FOREACH_PATTERN:
kv_foreach_pat_kernel runs the bytecode walk of kv_validate_kernel with a list element as the
root and feeds the verdict into the foreach reduction; reference pkg/engine/validation.go:156-283,
341-345, 421-445), on the bytecode VM and the specialized kernels. The expected side is the
decomposition of tests/foreach_pattern_data.py: the oracle for match / exclude, cond_model.py for
the preconditions, foreach_model.py for the list states and the reduction, and per element
`oracle.match_pattern` in its float mode.

Sizes 1, 63, 65, 257 and 513: resources 0 and 1 hold 300 and 70 containers, so their segments
straddle waves and workgroups; the lanes of one wave hold `ports` of 0-3 entries (the walk's loops
run the longest of them); the two lists differ in length."""
import os

import numpy as np
import pytest

import foreach_data as fd
import foreach_pattern_data as fpd
from kyverno_amd import batch, cli

pytestmark = pytest.mark.gpu
ENGINES = pytest.mark.parametrize("spec", [False, True], ids=["vm", "specialized"])
SIZES = [1, 63, 65, 257, 513]
KV_PATH_NONE = 0xFFFFFFFF
PATTERN_CASES = [c for c in fd.CASES if c["name"] in ("Test_foreach_container_pass", "Test_foreach_container_fail")]


@pytest.fixture(scope="module")
def crafted(orc):
    """Policy, resources and expected side of the crafted set at every size (computed once)."""
    pol = fpd.crafted_policy()
    sets = {}
    for n in SIZES:
        ress = fpd.crafted_resources(n)
        sets[n] = (ress, fpd.Expected(orc, pol, ress))
        sets[n][1].check_honest(full=n == 513)
    return pol, sets


def _evaluate(pol, ress, spec, mode=None, device_mask=None, pattern=True):
    """cli.evaluate with the result kept (statuses and messages of one kv_validate)."""
    ps = batch.PolicySet([pol], specialize=spec, foreach=True, foreach_pattern=pattern)
    b = batch.Batch(ps, ress)
    kw = {} if mode is None else {"mode": mode}
    r = batch.validate(ps, b, device_mask=device_mask, **kw)
    ev = cli.Evaluation([pol], ress, ps.rules, r.status)
    for ri, res in zip(*np.nonzero(r.status == cli.FAIL)):
        if ps.rules[ri].foreach:
            ev.foreach_elem[(int(ri), int(res))] = r.foreach_element(int(ri), int(res))
            if ps.rules[ri].foreach_pattern:
                ev.foreach_path[(int(ri), int(res))] = r.foreach_path(int(ri), int(res))
    cli.collect_errors(ev, ps, r, ress)
    return ps, b, r, ev


def _diff(names, got, want):
    bad = np.argwhere(got != want)
    return [(names[a], int(b), int(got[a, b]), int(want[a, b])) for a, b in bad[:20]]


def _element(rule, res, idx):
    """Element `idx` of the rule's list on the resource (request.object.<field>[.<field> | [i]]...)."""
    lst = res
    for k in rule["validate"]["foreach"][0]["list"].split(".")[2:]:
        if k.endswith("]"):
            k, i = k[:-1].split("[")
            lst = lst[k][int(i)]
        else:
            lst = lst[k]
    return (lst if isinstance(lst, list) else [lst])[idx]


# ------------------------------------------------------------------ the reference's own cases
@ENGINES
@pytest.mark.parametrize("case", PATTERN_CASES, ids=lambda c: c["name"])
def test_reference_cases(spec, case):
    """Test_foreach_container_pass / _fail (validation_test.go:2423-2505): status, deciding element
    and message."""
    assert len(PATTERN_CASES) == 2
    pol, res = case["policy"], case["resource"]
    ps, b, r, ev = _evaluate(pol, [res], spec)
    rule = ps.rules[0]
    assert (rule.route, rule.route_reason, rule.foreach, rule.foreach_pattern) == (batch.ROUTE_GPU, "", True, True)
    assert batch.STATUS_NAMES[int(r.status[0, 0])] == case["status"]
    if case["status"] == "pass":
        assert r.foreach_element(0, 0) is None and r.foreach_path(0, 0) is None
        assert cli.rule_message(ev, rule, 0) == "rule passed"
    else:  # pod2-invalid, the second container; the rule has no message (buildErrorMessage's first form)
        assert r.foreach_element(0, 0) == 1 and r.foreach_path(0, 0) == "/name/"
        assert r.foreach_error_message(0, 0, res["spec"]["template"]["spec"]["containers"][1]) == \
            "resource value 'pod2-invalid' does not match '*-valid' at path /name/"
        assert cli.rule_message(ev, rule, 0) == \
            "validation failed in foreach rule for validation error: rule test failed at path /name/"
    assert dict(r.phases).get("foreach", -1.0) >= 0.0


# ------------------------------------------------------------------ crafted parity
@ENGINES
@pytest.mark.parametrize("n", SIZES)
def test_crafted_parity(crafted, spec, n):
    pol, sets = crafted
    ress, exp = sets[n]
    rules = pol["spec"]["rules"]
    names = [x["name"] for x in rules]
    ps, b, r, ev = _evaluate(pol, ress, spec)
    assert [x.foreach_pattern for x in ps.rules] == [fpd.on_device(x) for x in rules]
    assert not _diff(names, r.status, exp.status)
    # the deciding element, the failing path inside it, the pattern error's text (the oracle's `msg`
    # in float mode) and the message of every FAIL / ERROR pair; "rule passed" / "rule skipped"
    fails = errors = 0
    for ri in range(len(names)):
        for k in range(n):
            st = int(exp.status[ri, k])
            assert r.foreach_element(ri, k) == exp.elem.get((ri, k)), (names[ri], k)
            assert r.foreach_path(ri, k) == exp.path.get((ri, k)), (names[ri], k)
            if (ri, k) in exp.elem:
                el = _element(rules[ri], ress[k], exp.elem[(ri, k)])
                assert r.foreach_error_message(ri, k, el) == exp.err[(ri, k)], (names[ri], k)
                fails += st == cli.FAIL
                errors += st == cli.ERROR
            if (ri, k) in exp.messages:
                assert cli.rule_message(ev, ps.rules[ri], k) == exp.messages[(ri, k)], (names[ri], k)
            if ps.rules[ri].foreach_pattern:
                assert r.foreach_message(ri, k) == ("rule skipped" if exp.messages.get((ri, k)) == "rule skipped" else None)
                assert r.deny_message(ri, k) is None
    assert n == 1 or (fails and errors)
    # kv_result_failures: every FAIL / ERROR / SKIP pair in order, no path id for foreach pairs
    frule, fres, fpid, _ = r.failures()
    want = [(a, c) for a in range(len(names)) for c in range(n) if exp.status[a, c] in (cli.FAIL, cli.ERROR, cli.SKIP)]
    assert list(zip(frule.tolist(), fres.tolist())) == want
    assert all(p == KV_PATH_NONE for p in fpid.tolist())
    assert all(r.path(a, c) is None for a, c in want[:50])


@ENGINES
def test_float_rendering_of_a_large_port(orc, spec):
    """An element with "port": 8080000 and no `tier` under {"(tier)": "ok", "port": "<1024"}: the value
    fails and the condition anchor's key is missing, an ERROR whose text renders the number as the
    reference's float64 element does (8.08e+06, not 8080000)."""
    pol = fpd.pd._policy("large-port", [fpd._rule("anchored", {"(tier)": "ok", "port": "<1024"}, "ports of {{element.name}}"),
                                         fpd._rule("plain", {"port": "<1024"})])
    res = {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "p", "namespace": "ns"},
           "spec": {"containers": [{"name": "c0", "port": 80, "tier": "ok"}, {"name": "c1", "port": 8080000}]}}
    exp = fpd.Expected(orc, pol, [res])
    assert [int(x) for x in exp.status[:, 0]] == [cli.ERROR, cli.FAIL] and exp.elem == {(0, 0): 1, (1, 0): 1}
    text = "resource value '8.08e+06' does not match '<1024' at path /port/"
    assert exp.err == {(0, 0): text, (1, 0): text}
    ps, b, r, ev = _evaluate(pol, [res], spec)
    el = res["spec"]["containers"][1]
    assert [int(x) for x in r.status[:, 0]] == [cli.ERROR, cli.FAIL]
    for ri in (0, 1):
        assert r.foreach_element(ri, 0) == 1
        assert r.foreach_error_message(ri, 0, el) == text
        assert cli.rule_message(ev, ps.rules[ri], 0) == exp.messages[(ri, 0)]
    assert r.foreach_path(0, 0) is None and r.foreach_path(1, 0) == "/port/"
    assert exp.messages[(0, 0)] == ("validation failed in foreach rule for validation error: ports of c1. "
                                    "Rule anchored execution error: " + text)


@ENGINES
def test_int_typed_values_route_the_pair(orc, spec):
    """A separate two-rule set, outside the CPU cap: {"port": "?0"} compares the number's text form.
    On int ports every matched pair with elements is CPU; on 0.5-style values it is evaluated."""
    pol = fpd.int_policy()
    for fl in (False, True):
        ress = fpd.crafted_resources(257, float_ports=fl)
        exp = fpd.Expected(orc, pol, ress)
        ps, b, r, ev = _evaluate(pol, ress, spec)
        assert not _diff(["port-glob", "name-set"], r.status, exp.status), fl
        row = exp.status[0][exp.status[0] != cli.NOMATCH]
        if fl:
            assert (row == cli.FAIL).any() and (row == cli.CPU).sum() * 5 < len(row)
        else:
            assert set(row.tolist()) <= {cli.CPU, cli.SKIP} and (row == cli.CPU).sum() * 2 > len(row)
        other = exp.status[1][exp.status[1] != cli.NOMATCH]
        assert (other == cli.PASS).sum() * 2 > len(other)  # (the string leaf beside it is evaluated)


@ENGINES
def test_typing_arms(orc, spec):
    """The other arms of the int-typing guard: |n| >= 2^53 under a number pattern (2^53 - 1 is
    evaluated), an int inside a nested list under a glob, ints in a scalar list (the leaf that
    walks every element)."""
    pol, ress = fpd.typing_policy(), fpd.typing_resources()
    exp = fpd.Expected(orc, pol, ress)
    C, F, P = cli.CPU, cli.FAIL, cli.PASS
    assert exp.status[0, 1:4].tolist() == [C, F, C] and exp.status[1, 4:7].tolist() == [C, P, F]
    assert exp.status[2, 7:10].tolist() == [P, C, F] and exp.status[3, 7:12].tolist() == [C, C, P, C, P]
    ps, b, r, ev = _evaluate(pol, ress, spec)
    assert not _diff([x["name"] for x in pol["spec"]["rules"]], r.status, exp.status)
    for (ri, k), el in exp.elem.items():
        assert r.foreach_element(ri, k) == el and r.foreach_path(ri, k) == exp.path.get((ri, k))
        assert r.foreach_error_message(ri, k, ress[k]["spec"]["containers"][el]) == exp.err[(ri, k)]


@ENGINES
def test_counts_and_scopes(crafted, spec):
    pol, sets = crafted
    ress, exp = sets[513]
    ps = batch.PolicySet([pol], specialize=spec, foreach=True, foreach_pattern=True)
    b = batch.Batch(ps, ress)
    r = batch.validate(ps, b, mode=batch.MODE_COUNTS | batch.MODE_SCOPES)
    want = exp.counts()
    assert np.array_equal(np.asarray(r.counts).reshape(want.shape[0], -1)[:, :7], want[:, :7])
    ns = list(b.namespaces)
    sc = np.asarray(r.scope_counts).reshape(len(ns), want.shape[0], -1)
    for si, name in enumerate(ns):
        sel = np.array([x["metadata"].get("namespace", "") == name for x in ress])
        for s in range(7):
            assert np.array_equal(sc[si, :, s], (exp.status[:, sel] == s).sum(axis=1)), (name, s)


@ENGINES
def test_parts_match_one_batch(crafted, spec):
    """The 513 set as three logical parts of one device: each part walks its own elements and
    carries its own key and record rows."""
    pol, sets = crafted
    ress, exp = sets[513]
    rules = pol["spec"]["rules"]
    names = [x["name"] for x in rules]
    old = os.environ.get("KVGPU_SHARDS_PER_DEVICE")
    os.environ["KVGPU_SHARDS_PER_DEVICE"] = "3"
    try:
        ps, b, r, ev = _evaluate(pol, ress, spec, device_mask=1)
    finally:
        if old is None:
            os.environ.pop("KVGPU_SHARDS_PER_DEVICE", None)
        else:
            os.environ["KVGPU_SHARDS_PER_DEVICE"] = old
    assert not _diff(names, r.status, exp.status)
    for (ri, k), el in exp.elem.items():
        assert r.foreach_element(ri, k) == el, (names[ri], k)
        assert r.foreach_path(ri, k) == exp.path.get((ri, k)), (names[ri], k)
        assert r.foreach_error_message(ri, k, _element(rules[ri], ress[k], el)) == exp.err[(ri, k)], (names[ri], k)
    assert np.array_equal(np.asarray(r.counts).reshape(len(names), -1)[:, :7], exp.counts()[:, :7])


@ENGINES
def test_flag_off_is_cpu(crafted, spec):
    """The same policy compiled with KV_COMPILE_FOREACH alone: CPU for every matched pair."""
    pol, sets = crafted
    ress, exp = sets[257]
    ps, b, r, ev = _evaluate(pol, ress, spec, pattern=False)
    want = np.where(exp.status == cli.NOMATCH, cli.NOMATCH, cli.CPU)
    assert np.array_equal(r.status, want)
    assert not any(x.foreach or x.foreach_pattern for x in ps.rules)
    assert "foreach" not in dict(r.phases)


@ENGINES
def test_foreach_phase(crafted, spec):
    pol, sets = crafted
    ress, _ = sets[65]
    ps, b, r, ev = _evaluate(pol, ress, spec)
    phases = dict(r.phases)
    assert phases.get("foreach", -1.0) >= 0.0
    assert phases.get("precond", -1.0) >= 0.0  # (the crafted set has a rule-level precondition too)
    assert "deny" not in phases
