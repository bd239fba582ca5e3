"""validate.foreach on the device (KV_COMPILE_FOREACH: kv_foreach_elem_kernel and
kv_foreach_fin_kernel, consumed by both engines through the deny plane; reference
pkg/engine/validation.go:204-283), on the bytecode VM and the specialized kernels. The oracle
reports foreach rules as CPU, so the expected side is the decomposition of tests/foreach_data.py:
the oracle for match / exclude, cond_model.py for the rule's preconditions, foreach_model.py for
the entry."""
import os

import numpy as np
import pytest

import foreach_data as fd
from kyverno_amd import batch, cli

pytestmark = pytest.mark.gpu
ENGINES = pytest.mark.parametrize("spec", [False, True], ids=["vm", "specialized"])
SIZES = [1, 63, 65, 257, 513]
KV_PATH_NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def crafted(orc):
    """Policy, resources and expected side of the crafted set at every size (computed once)."""
    pol = fd.crafted_policy()
    sets = {}
    for n in SIZES:
        ress = fd.crafted_resources(n)
        sets[n] = (ress, fd.Expected(orc, pol, ress))
        sets[n][1].check_honest(full=n == 513)
    return pol, sets


def _evaluate(pol, ress, spec, mode=None, device_mask=None, foreach=True):
    """cli.evaluate with the result kept (statuses and messages of one kv_validate)."""
    ps = batch.PolicySet([pol], specialize=spec, foreach=foreach)
    b = batch.Batch(ps, ress)
    kw = {} if mode is None else {"mode": mode}
    r = batch.validate(ps, b, device_mask=device_mask, **kw)
    ev = cli.Evaluation([pol], ress, ps.rules, r.status)
    for ri, res in zip(*np.nonzero(r.status == cli.FAIL)):
        if ps.rules[ri].foreach:
            ev.foreach_elem[(int(ri), int(res))] = r.foreach_element(int(ri), int(res))
    cli.collect_errors(ev, ps, r, ress)
    return ps, b, r, ev


def _diff(names, got, want):
    bad = np.argwhere(got != want)
    return [(names[a], int(b), int(got[a, b]), int(want[a, b])) for a, b in bad[:20]]


# ------------------------------------------------------------------ golden end to end
@ENGINES
@pytest.mark.parametrize("case", fd.CASES, ids=lambda c: c["name"])
def test_golden_cases(spec, case):
    pol, res = case["policy"], case["resource"]
    ps, b, r, ev = _evaluate(pol, [res], spec)
    st = int(r.status[0, 0])
    if case["device"]["route"] == "cpu":  # regex_match / pattern: left to the reference engine
        assert (ps.rules[0].route, ps.rules[0].route_reason) == (batch.ROUTE_CPU, "foreach") and st == cli.CPU
        return
    assert (ps.rules[0].route, ps.rules[0].route_reason, ps.rules[0].foreach) == (batch.ROUTE_GPU, "", True)
    assert batch.STATUS_NAMES[st] == case["status"]
    assert cli.rule_message(ev, ps.rules[0], 0) == case["message"]
    assert r.foreach_element(0, 0) == case["element"]
    assert dict(r.phases).get("foreach", -1.0) >= 0.0


# ------------------------------------------------------------------ crafted parity
@ENGINES
@pytest.mark.parametrize("n", SIZES)
def test_crafted_parity(crafted, spec, n):
    pol, sets = crafted
    ress, exp = sets[n]
    names = [x["name"] for x in pol["spec"]["rules"]]
    ps, b, r, ev = _evaluate(pol, ress, spec)
    assert [x.foreach for x in ps.rules] == [fd.on_device(x) for x in pol["spec"]["rules"]]
    assert not _diff(names, r.status, exp.status)
    # the message of every FAIL / ERROR / SKIP / PASS foreach pair (an ERROR text only where exactly
    # one string of the block is unresolved: with several, which one the reference meets first is
    # Go's map order)
    compared = 0
    for (ri, k), msgs in exp.messages.items():
        got = cli.rule_message(ev, ps.rules[ri], k)
        if len(msgs) == 1:
            assert got == msgs[0], (names[ri], k)
            compared += 1
        else:
            assert got in msgs, (names[ri], k)
        assert r.deny_message(ri, k) is None, (names[ri], k)  # (stays 0 for foreach rules)
        assert (r.precond_message(ri, k) == fd.NOT_MET) == bool(exp.gated[ri, k]), (names[ri], k)
        st = int(r.status[ri, k])
        fm = r.foreach_message(ri, k)
        if st == cli.ERROR:
            assert fm is not None and fm in msgs
        elif st == cli.SKIP:
            assert fm == (None if exp.gated[ri, k] else "rule skipped"), (names[ri], k)
        else:
            assert fm is None, (names[ri], k)
    assert compared
    # the deciding element: the model's, and the host fold's
    fst, fel = ps.foreach_fold(b)
    rule_sets = ps.foreach_info["rule_sets"]
    for ri in range(len(names)):
        for k in range(n):
            got = r.foreach_element(ri, k)
            assert got == exp.elem.get((ri, k)), (names[ri], k)
            if got is not None:
                assert got == int(fel[rule_sets[ri] - 1, k]) and r.status[ri, k] == fst[rule_sets[ri] - 1, k]
    # kv_result_failures: every FAIL / ERROR / SKIP pair in order; a foreach pair has no path, and
    # its SKIP owns a slot with an empty record as a gated SKIP does
    frule, fres, fpid, fpaths = r.failures()
    want = [(a, c) for a in range(len(names)) for c in range(n) if exp.status[a, c] in (cli.FAIL, cli.ERROR, cli.SKIP)]
    assert list(zip(frule.tolist(), fres.tolist())) == want
    for a, c, p in zip(frule.tolist(), fres.tolist(), fpid.tolist()):
        if ps.rules[a].foreach:
            assert p == KV_PATH_NONE, (names[a], c)
            assert r.path(a, c) is None
        elif exp.status[a, c] == cli.FAIL:
            assert p != KV_PATH_NONE


@ENGINES
def test_counts_and_scopes(crafted, spec):
    pol, sets = crafted
    ress, exp = sets[513]
    ps = batch.PolicySet([pol], specialize=spec, foreach=True)
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
    """The 513 set as three logical parts of one device: each part carries its slice of the
    element rows (the elements of a resource stay together) and its own plane."""
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
            assert r.foreach_message(ri, k) in msgs, (names[ri], k)
        if (ri, k) in exp.elem:
            assert r.foreach_element(ri, k) == exp.elem[(ri, k)], (names[ri], k)
    assert np.array_equal(np.asarray(r.counts).reshape(len(names), -1)[:, :7], exp.counts()[:, :7])


@ENGINES
def test_foreach_phase(crafted, spec):
    pol, sets = crafted
    ress, _ = sets[65]
    ps, b, r, ev = _evaluate(pol, ress, spec)
    phases = dict(r.phases)
    assert phases.get("foreach", -1.0) >= 0.0
    assert phases.get("precond", -1.0) >= 0.0  # (the crafted set has a rule-level precondition too)
    assert "deny" not in phases


@ENGINES
def test_flag_off_is_cpu(crafted, spec):
    """The same policy compiled without the flag: CPU for every matched foreach pair."""
    pol, sets = crafted
    ress, exp = sets[257]
    ps, b, r, ev = _evaluate(pol, ress, spec, foreach=False)
    for ri, rule in enumerate(pol["spec"]["rules"]):
        if fd.is_foreach(rule):
            want = np.where(exp.status[ri] == cli.NOMATCH, cli.NOMATCH, cli.CPU)
            assert np.array_equal(r.status[ri], want), rule["name"]
        else:
            assert np.array_equal(r.status[ri], exp.status[ri]), rule["name"]
    assert "foreach" not in dict(r.phases)
