"""validate.foreach rules of several entries on the device (KV_COMPILE_FOREACH_ENTRIES: the entry
sets through kv_foreach_elem_kernel / kv_foreach_pat_kernel, then kv_foreach_chain_kernel, consumed
by both engines through the deny plane; reference pkg/engine/validation.go:204-283), on the
bytecode VM and the specialized kernels. The oracle reports foreach rules as CPU, so the expected
side is the decomposition of tests/foreach_chain_data.py: the oracle for match / exclude,
cond_model.py for the rule's preconditions, foreach_chain_model.py for the entries."""
import os

import numpy as np
import pytest

import foreach_chain_data as cd
from kyverno_amd import batch, cli

pytestmark = pytest.mark.gpu
ENGINES = pytest.mark.parametrize("spec", [False, True], ids=["vm", "specialized"])
SIZES = [1, 63, 65, 257, 513]
KV_PATH_NONE = 0xFFFFFFFF
ALL = {"foreach": True, "foreach_pattern": True, "foreach_entries": True}


@pytest.fixture(scope="module")
def crafted(orc):
    """Policy, resources and expected side of the crafted set at every size (computed once)."""
    pol = cd.crafted_policy()
    sets = {}
    for n in SIZES:
        ress = cd.crafted_resources(n)
        sets[n] = (ress, cd.Expected(orc, pol, ress))
    sets[257][1].check_cases()
    sets[513][1].check_cases()
    return pol, sets


def _evaluate(pol, ress, spec, mode=None, device_mask=None, flags=ALL):
    """cli.evaluate with the result kept (statuses and messages of one kv_validate)."""
    ps = batch.PolicySet([pol], specialize=spec, **flags)
    b = batch.Batch(ps, ress)
    kw = {} if mode is None else {"mode": mode}
    r = batch.validate(ps, b, device_mask=device_mask, **kw)
    ev = cli.Evaluation([pol], ress, ps.rules, r.status)
    for ri, res in zip(*np.nonzero(r.status == cli.FAIL)):
        if ps.rules[ri].foreach:
            key = (int(ri), int(res))
            ev.foreach_elem[key] = r.foreach_element(*key)
            if ps.rules[ri].foreach_entries:
                ev.foreach_entry[key] = r.foreach_entry(*key)
            if cli._pattern_entry(ev, ps.rules[ri], key[1]):
                ev.foreach_path[key] = r.foreach_path(*key)
    cli.collect_errors(ev, ps, r, ress)
    return ps, b, r, ev


def _diff(names, got, want):
    bad = np.argwhere(got != want)
    return [(names[a], int(b), int(got[a, b]), int(want[a, b])) for a, b in bad[:20]]


# ------------------------------------------------------------------ golden end to end
@ENGINES
@pytest.mark.parametrize("case", cd.CASES_GOLDEN, ids=lambda c: c["name"])
def test_golden_cases(spec, case):
    pol, res = case["policy"], case["resource"]
    ps, b, r, ev = _evaluate(pol, [res], spec)
    st = int(r.status[0, 0])
    if case["device"]["route"] == "cpu":  # `..` in the second list: left to the reference engine
        assert (ps.rules[0].route, ps.rules[0].route_reason) == (batch.ROUTE_CPU, "foreach") and st == cli.CPU
        return
    assert (ps.rules[0].route, ps.rules[0].route_reason, ps.rules[0].foreach, ps.rules[0].foreach_entries) == \
        (batch.ROUTE_GPU, "", True, 2)
    assert batch.STATUS_NAMES[st] == case["status"]
    assert cli.rule_message(ev, ps.rules[0], 0) == case["message"]
    assert r.foreach_entry(0, 0) == case["entry"] and r.foreach_element(0, 0) == case["element"]
    assert dict(r.phases).get("foreach", -1.0) >= 0.0


# ------------------------------------------------------------------ crafted parity
@ENGINES
@pytest.mark.parametrize("n", SIZES)
def test_crafted_parity(crafted, spec, n):
    pol, sets = crafted
    ress, exp = sets[n]
    names = [x["name"] for x in pol["spec"]["rules"]]
    ps, b, r, ev = _evaluate(pol, ress, spec)
    assert [x.foreach for x in ps.rules] == [cd.on_device(x) for x in pol["spec"]["rules"]]
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
        assert (r.precond_message(ri, k) == cd.NOT_MET) == bool(exp.gated[ri, k]), (names[ri], k)
        st = int(r.status[ri, k])
        fm = r.foreach_message(ri, k)
        if st == cli.ERROR and (ri, k) not in exp.err:  # (a deny entry's; a pattern entry's is its pattern error)
            assert fm is not None and fm in msgs
        elif st == cli.SKIP:
            assert fm == (None if exp.gated[ri, k] else "rule skipped"), (names[ri], k)
        else:
            assert fm is None, (names[ri], k)
    assert compared
    # the deciding entry and element, and the failing path inside it where a pattern entry decided
    for ri in range(len(names)):
        single = ps.rules[ri].foreach and not ps.rules[ri].foreach_entries
        for k in range(n):
            assert r.foreach_element(ri, k) == exp.elem.get((ri, k)), (names[ri], k)
            want = exp.entry.get((ri, k))
            assert r.foreach_entry(ri, k) == want, (names[ri], k)
            assert want is None or not single or want == 0
            assert r.foreach_path(ri, k) == exp.path.get((ri, k)), (names[ri], k)
    # the host fold of the chains without a pattern entry
    fst, fen, fel = ps.foreach_chain_fold(b)
    chains = ps.foreach_chain_info["rule_chains"]
    for ri, name in enumerate(names):
        if not chains[ri] or name in cd.PATTERN_RULES:
            continue
        for k in range(n):
            if (ri, k) in exp.elem:
                c = chains[ri] - 1
                assert (int(fst[c, k]), int(fen[c, k]), int(fel[c, k])) == \
                    (int(r.status[ri, k]), exp.entry[(ri, k)], exp.elem[(ri, k)]), (name, k)
    # kv_result_failures: every FAIL / ERROR / SKIP pair in order; a foreach pair has no path
    frule, fres, fpid, fpaths = r.failures()
    want = [(a, c) for a in range(len(names)) for c in range(n) if exp.status[a, c] in (cli.FAIL, cli.ERROR, cli.SKIP)]
    assert list(zip(frule.tolist(), fres.tolist())) == want
    for a, c, p in zip(frule.tolist(), fres.tolist(), fpid.tolist()):
        if ps.rules[a].foreach:
            assert p == KV_PATH_NONE, (names[a], c)
            assert r.path(a, c) is None


@ENGINES
def test_counts_and_scopes(crafted, spec):
    pol, sets = crafted
    ress, exp = sets[513]
    ps = batch.PolicySet([pol], specialize=spec, **ALL)
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
    """The 513 set as three logical parts of one device: each part carries its slice of the element
    rows of every (list, context), its own plane and its own chain keys."""
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
        if exp.status[ri, k] == cli.ERROR and (ri, k) not in exp.err:
            assert r.foreach_message(ri, k) in msgs, (names[ri], k)
        if (ri, k) in exp.elem:
            assert (r.foreach_entry(ri, k), r.foreach_element(ri, k)) == (exp.entry[(ri, k)], exp.elem[(ri, k)]), (names[ri], k)
            assert r.foreach_path(ri, k) == exp.path.get((ri, k)), (names[ri], k)
            if len(msgs) == 1:
                assert cli.rule_message(ev, ps.rules[ri], k) == msgs[0], (names[ri], k)
    assert np.array_equal(np.asarray(r.counts).reshape(len(names), -1)[:, :7], exp.counts()[:, :7])


@ENGINES
def test_flag_off_is_cpu(crafted, spec):
    """The same policy compiled without the new flag: every rule of several entries is (CPU,
    "foreach") and its matched pairs are CPU; the rule of one entry is evaluated as before."""
    pol, sets = crafted
    ress, exp = sets[257]
    ps, b, r, ev = _evaluate(pol, ress, spec, flags={"foreach": True, "foreach_pattern": True})
    for ri, rule in enumerate(pol["spec"]["rules"]):
        if cd.is_chain(rule):
            assert (ps.rules[ri].route, ps.rules[ri].route_reason) == (batch.ROUTE_CPU, "foreach"), rule["name"]
            want = np.where(exp.status[ri] == cli.NOMATCH, cli.NOMATCH, cli.CPU)
            assert np.array_equal(r.status[ri], want), rule["name"]
        else:
            assert np.array_equal(r.status[ri], exp.status[ri]), rule["name"]
