"""Rule preconditions on the device (kv_precond_kernel, the gate of both engines; reference
pkg/engine/validation.go:175-193, variables/evaluate.go:42-78, variables/operator/*.go), on the
bytecode VM and the specialized kernels. The oracle reports such rules as CPU, so the expected
side is the decomposition of tests/precond_data.py: the oracle on the rule without its
preconditions, gated by the model (tests/cond_model.py)."""
import io
import json
import os

import numpy as np
import pytest

import cond_model
import precond_data as pd
from kyverno_amd import batch, cli

pytestmark = pytest.mark.gpu
ENGINES = pytest.mark.parametrize("spec", [False, True], ids=["vm", "specialized"])
SIZES = [1, 63, 65, 513]


@pytest.fixture(scope="module")
def crafted(orc):
    """Policy, resources and expected side of the crafted set at every size (computed once)."""
    pol = pd.crafted_policy()
    return pol, {n: (pd.crafted_resources(n), pd.Expected(orc, pol, pd.crafted_resources(n))) for n in SIZES}


def _evaluate(pol, ress, spec, mode=None, device_mask=None):
    """cli.evaluate with the result kept (statuses, paths, messages of one kv_validate)."""
    ps = batch.PolicySet([pol], specialize=spec)
    b = batch.Batch(ps, ress)
    kw = {} if mode is None else {"mode": mode}
    r = batch.validate(ps, b, device_mask=device_mask, **kw)
    ev = cli.Evaluation([pol], ress, ps.rules, r.status)
    for ri, res in zip(*np.nonzero(r.status == cli.FAIL)):
        if not ps.rules[ri].any_pattern:
            ev.paths[(int(ri), int(res))] = r.path(int(ri), int(res))
    cli.collect_errors(ev, ps, r, ress)
    cli._evaluate_anypatterns(ev, 0, spec)
    return ps, b, r, ev


def _diff(names, got, want):
    bad = np.argwhere(got != want)
    return [(names[a], int(b), int(got[a, b]), int(want[a, b])) for a, b in bad[:20]]


# ------------------------------------------------------------------ golden table end to end
@ENGINES
def test_golden_table_end_to_end(orc, spec):
    """One rule per in-scope row of the reference's TestEvaluate over 257 resources (a full
    256-lane workgroup and a one-lane tail): even resources carry every operand, odd ones none."""
    pol, ress = pd.golden_policy(), pd.golden_resources(257)
    exp = pd.golden_expected(cond_model.Model(orc), 257)
    ps = batch.PolicySet([pol], specialize=spec)
    assert all(r.route == batch.ROUTE_GPU for r in ps.rules)
    r = batch.validate(ps, batch.Batch(ps, ress))
    names = [x["name"] for x in pol["spec"]["rules"]]
    assert not _diff(names, r.status, exp)
    assert (exp[:, 1] != exp[:, 0]).any()  # neighbouring lanes disagree
    skip = np.argwhere(r.status == cli.SKIP)
    for a, c in skip[:: max(1, len(skip) // 200)]:
        assert r.precond_message(int(a), int(c)) == pd.NOT_MET
    assert dict(r.phases).get("precond", -1.0) >= 0.0


# ------------------------------------------------------------------ crafted parity
@ENGINES
@pytest.mark.parametrize("n", SIZES)
def test_crafted_parity(crafted, spec, n):
    pol, sets = crafted
    ress, exp = sets[n]
    names = [x["name"] for x in pol["spec"]["rules"]]
    ps, b, r, ev = _evaluate(pol, ress, spec)
    assert [(x.route, x.route_reason) for x in ps.rules] == [(batch.ROUTE_GPU, "")] * len(names)
    assert not _diff(names, r.status, exp.status)
    if n == 513:  # both ends of an undecided condition occur (an array operand)
        aa = names.index("any-all-array")
        arr = np.array([isinstance(x["spec"].get("zones"), list) for x in ress])
        assert (r.status[aa][arr] == cli.CPU).any() and (r.status[aa][arr] != cli.CPU).any()
    # path and message of every FAIL / SKIP / ERROR pair
    rules = {x.index: x for x in ps.rules}
    for ri, k in np.argwhere((r.status == cli.FAIL) | (r.status == cli.SKIP) | (r.status == cli.ERROR)):
        ri, k = int(ri), int(k)
        path, msg = exp.detail(ri, k)
        assert cli.rule_message(ev, rules[ri], k) == msg, (names[ri], k)
        if r.status[ri, k] == cli.FAIL and not rules[ri].any_pattern:
            assert r.path(ri, k) == path, (names[ri], k)
        assert (r.precond_message(ri, k) == pd.NOT_MET) == bool(exp.gated[ri, k]), (names[ri], k)
        assert exp.gated[ri, k] == ((ri, k) in ev.precond)
    # kv_result_failures: every FAIL / ERROR / SKIP pair in order, a precondition SKIP without a path
    frule, fres, fpid, fpaths = r.failures()
    want = [(a, c) for a in range(len(names)) for c in range(n) if exp.status[a, c] in (cli.FAIL, cli.ERROR, cli.SKIP)]
    assert list(zip(frule.tolist(), fres.tolist())) == want
    for a, c, p in zip(frule.tolist(), fres.tolist(), fpid.tolist()):
        if exp.gated[a, c]:
            assert p == 0xFFFFFFFF
        elif exp.status[a, c] == cli.FAIL:
            assert p != 0xFFFFFFFF
            if not rules[a].any_pattern:
                assert fpaths[p] == exp.detail(a, c)[0]


@ENGINES
def test_cause_is_attributed(crafted, spec):
    """On the conditional-anchor rule a SKIP of the pattern's anchor is not the preconditions'."""
    pol, sets = crafted
    ress, exp = sets[513]
    names = [x["name"] for x in pol["spec"]["rules"]]
    ca = names.index("conditional-anchor")
    ps, b, r, ev = _evaluate(pol, ress, spec)
    skip = np.nonzero(r.status[ca] == cli.SKIP)[0]
    gated = [int(k) for k in skip if exp.gated[ca, k]]
    anchor = [int(k) for k in skip if not exp.gated[ca, k]]
    assert gated and anchor
    for k in gated:
        assert r.precond_message(ca, k) == pd.NOT_MET
        assert r.error_message(ca, k, ress[k]) is None  # kv_result_error_message: KV_E_INVALID
    for k in anchor:
        assert r.precond_message(ca, k) is None
        assert cli.rule_message(ev, ps.rules[ca], k) == exp.detail(ca, k)[1] != pd.NOT_MET
    # other statuses have no precondition message
    k = int(np.nonzero(r.status[ca] == cli.PASS)[0][0])
    assert r.precond_message(ca, k) is None


@ENGINES
def test_counts_and_scopes(crafted, spec):
    pol, sets = crafted
    ress, exp = sets[513]
    ps = batch.PolicySet([pol], specialize=spec)
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
    """The 513 set as three logical parts of one device: a 64-aligned shard cut falls inside the
    batch, and each part carries its slice of the condition outcomes."""
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
    for ri, k in np.argwhere(r.status == cli.SKIP):
        assert (r.precond_message(int(ri), int(k)) == pd.NOT_MET) == bool(exp.gated[ri, k])
    assert np.array_equal(np.asarray(r.counts).reshape(len(names), -1)[:, :7], exp.counts()[:, :7])


# ------------------------------------------------------------------ CLI
@ENGINES
def test_cli_preconditions_case(spec, tmp_path):
    """test/cli/test/preconditions: test-valid passes, test-invalid fails with the reference's
    message form; a third Pod labelled app=other is skipped, "preconditions not met"."""
    case = pd.CLI_CASE
    other = json.loads(json.dumps(case["resources"][1]))
    other["metadata"]["name"] = "test-other"
    other["metadata"]["labels"]["app"] = "other"
    ress = case["resources"] + [other]
    rows = cli.run_test({"results": case["results"] + [{"policy": "preconditions", "rule": "any-rule",
                                                        "resource": "test-other", "kind": "Pod", "status": "skip"}]},
                        case["policies"], ress,
                        evaluation_fn=lambda p, r: cli.evaluate(p, r, messages=False, specialize=spec))
    assert [(x["resource"], x["actual"], x["ok"]) for x in rows] == \
        [("test-valid", "pass", True), ("test-invalid", "fail", True), ("test-other", "skip", True)]
    out = io.StringIO()
    rc, infos = cli.apply_docs(case["policies"], ress, out=out,
                               evaluation_fn=lambda p, r: cli.evaluate(p, r, specialize=spec))
    assert (rc.pass_, rc.fail, rc.error, rc.routed) == (1, 1, 0, 0)
    by = {i["resource"]["name"]: i["rules"][0] for i in infos}
    assert by["test-valid"]["status"] == "pass"
    assert by["test-invalid"] == {
        "name": "any-rule", "status": "fail",
        "message": "validation error: Busybox must be used based on this label combination. Rule any-rule failed at "
                   "path /spec/containers/0/name/"}
    assert by["test-other"] == {"name": "any-rule", "status": "skip", "message": pd.NOT_MET}
    assert "routed to the reference engine" not in out.getvalue()
