"""validate.deny on the device (KV_COMPILE_DENY: kv_deny_kernel, consumed by both engines; reference
pkg/engine/validation.go:299-339), on the bytecode VM and the specialized kernels. The oracle
reports deny rules as CPU, so the expected side is the decomposition of tests/deny_data.py: the
oracle for match / exclude, cond_model.py for the preconditions, deny_model.py for the block."""
import os

import numpy as np
import pytest

import deny_data as dd
from kyverno_amd import batch, cli

pytestmark = pytest.mark.gpu
ENGINES = pytest.mark.parametrize("spec", [False, True], ids=["vm", "specialized"])
SIZES = [1, 63, 65, 257, 513]
KV_PATH_NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def crafted(orc):
    """Policy, resources and expected side of the crafted set at every size (computed once)."""
    pol = dd.crafted_policy()
    sets = {}
    for n in SIZES:
        ress = dd.crafted_resources(n)
        sets[n] = (ress, dd.Expected(orc, pol, ress))
        sets[n][1].check_honest(full=n == 513)
    return pol, sets


def _evaluate(pol, ress, spec, mode=None, device_mask=None):
    """cli.evaluate with the result kept (statuses and messages of one kv_validate)."""
    ps = batch.PolicySet([pol], specialize=spec, deny=True)
    b = batch.Batch(ps, ress)
    kw = {} if mode is None else {"mode": mode}
    r = batch.validate(ps, b, device_mask=device_mask, **kw)
    ev = cli.Evaluation([pol], ress, ps.rules, r.status)
    cli.collect_errors(ev, ps, r, ress)
    return ps, b, r, ev


def _diff(names, got, want):
    bad = np.argwhere(got != want)
    return [(names[a], int(b), int(got[a, b]), int(want[a, b])) for a, b in bad[:20]]


# ------------------------------------------------------------------ golden end to end
@ENGINES
@pytest.mark.parametrize("case", dd.CASES, ids=lambda c: c["name"])
def test_golden_cases(orc, spec, case):
    pol, res = case["policy"], case["resource"]
    exp = dd.Expected(orc, pol, [res])
    ps, b, r, ev = _evaluate(pol, [res], spec)
    assert (ps.rules[0].route, ps.rules[0].route_reason, ps.rules[0].deny) == (batch.ROUTE_GPU, "", True)
    st = int(r.status[0, 0])
    assert st == exp.status[0, 0]
    assert (st in (cli.PASS, cli.SKIP)) == case["successful"]
    assert [cli.rule_message(ev, ps.rules[0], 0)] == exp.messages[(0, 0)]
    if case["status"] is not None:  # the reference's own assertions on Rules[0]
        assert batch.STATUS_NAMES[st] == case["status"]
        assert cli.rule_message(ev, ps.rules[0], 0) == case["message"]
    if case["name"] == "VariablesInMessageAreResolved":
        assert cli.rule_message(ev, ps.rules[0], 0) == "The animal cow is not in the allowed list of animals."
    assert dict(r.phases).get("deny", -1.0) >= 0.0


@ENGINES
def test_cli_duration_case(spec):
    """test/cli/test/simple with deny=True: the 5 rows of today plus the four duration-test rows
    (fail / pass / fail / pass), none routed to the reference engine."""
    case = dd.CLI_SIMPLE
    rows = cli.run_test(case, case["policies"], case["resources"],
                        evaluation_fn=lambda p, r: cli.evaluate(p, r, messages=False, specialize=spec, deny=True))
    assert not [x for x in rows if x["ok"] is not True], [x for x in rows if x["ok"] is not True]
    assert len(rows) == 9
    dur = [(x["rule"], x["actual"]) for x in rows if x["policy"] == "duration-test"]
    assert dur == [("greater-than", "fail"), ("less-than", "pass"), ("greater-equal-than", "fail"),
                   ("less-equal-than", "pass")]
    # without the flag the same four rows are routed, as tests/test_cli.py pins
    rows = cli.run_test(case, case["policies"], case["resources"],
                        evaluation_fn=lambda p, r: cli.evaluate(p, r, messages=False, specialize=spec))
    assert sum(x["ok"] is True for x in rows) == 5 and sum(x["ok"] is None for x in rows) == 4


# ------------------------------------------------------------------ crafted parity
@ENGINES
@pytest.mark.parametrize("n", SIZES)
def test_crafted_parity(crafted, spec, n):
    pol, sets = crafted
    ress, exp = sets[n]
    names = [x["name"] for x in pol["spec"]["rules"]]
    ps, b, r, ev = _evaluate(pol, ress, spec)
    assert [(x.route, x.route_reason) for x in ps.rules] == [(batch.ROUTE_GPU, "")] * len(names)
    assert [x.deny for x in ps.rules] == [dd.is_deny(x) for x in pol["spec"]["rules"]]
    assert not _diff(names, r.status, exp.status)
    # message of every FAIL / ERROR / SKIP / PASS deny pair (an ERROR text only where exactly one
    # string of the block is unresolved: with several, which one the reference meets first is
    # Go's map order)
    compared = 0
    for (ri, k), msgs in exp.messages.items():
        got = cli.rule_message(ev, ps.rules[ri], k)
        if len(msgs) == 1:
            assert got == msgs[0], (names[ri], k)
            compared += 1
        else:
            assert got in msgs, (names[ri], k)
        st = int(r.status[ri, k])
        assert (r.deny_message(ri, k) is not None) == (st == cli.ERROR), (names[ri], k)
        assert (r.precond_message(ri, k) == dd.NOT_MET) == bool(exp.gated[ri, k]), (names[ri], k)
    assert compared
    # deny_message: None for other causes (the plain pattern rule, CPU / NOMATCH pairs)
    pp = names.index("plain-pattern")
    for k in range(min(n, 40)):
        assert r.deny_message(pp, k) is None
    for ri, k in np.argwhere((r.status == cli.CPU) | (r.status == cli.NOMATCH))[:40]:
        assert r.deny_message(int(ri), int(k)) is None
    # kv_result_failures: every FAIL / ERROR / SKIP pair in order; a deny pair has no path
    frule, fres, fpid, fpaths = r.failures()
    want = [(a, c) for a in range(len(names)) for c in range(n) if exp.status[a, c] in (cli.FAIL, cli.ERROR, cli.SKIP)]
    assert list(zip(frule.tolist(), fres.tolist())) == want
    for a, c, p in zip(frule.tolist(), fres.tolist(), fpid.tolist()):
        if ps.rules[a].deny:
            assert p == KV_PATH_NONE, (names[a], c)
            assert r.path(a, c) is None  # (kv_result_path: as for a gated SKIP)
        elif exp.status[a, c] == cli.FAIL:
            assert p != KV_PATH_NONE


@ENGINES
def test_counts_and_scopes(crafted, spec):
    pol, sets = crafted
    ress, exp = sets[513]
    ps = batch.PolicySet([pol], specialize=spec, deny=True)
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
    """The 513 set as three logical parts of one device: each part carries its slice of the deny
    outcomes and its own deny plane."""
    pol, sets = crafted
    ress, exp = sets[513]
    names = [x["name"] for x in pol["spec"]["rules"]]
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
    for (ri, k), msgs in exp.messages.items():
        if exp.status[ri, k] == cli.ERROR:
            assert r.deny_message(ri, k) in msgs, (names[ri], k)
    assert np.array_equal(np.asarray(r.counts).reshape(len(names), -1)[:, :7], exp.counts()[:, :7])


@ENGINES
def test_deny_phase(crafted, spec):
    pol, sets = crafted
    ress, _ = sets[65]
    ps, b, r, ev = _evaluate(pol, ress, spec)
    phases = dict(r.phases)
    assert phases.get("deny", -1.0) >= 0.0
    assert phases.get("precond", -1.0) >= 0.0  # (the crafted set has preconditions too)
