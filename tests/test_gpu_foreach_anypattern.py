"""validate.foreach entries with an `anyPattern` on the device (KV_COMPILE_FOREACH_ANYPATTERN:
kv_foreach_any_kernel tries the alternatives in order per element, each a pattern walk with the
element as the root, and feeds the verdict into the foreach reduction; kv_foreach_anyrec_kernel keeps
every alternative's outcome on the deciding element; reference pkg/engine/validation.go:175-202,
447-489, 536-547), on the bytecode VM and the specialized kernels. The expected side is the model
of tests/foreach_anypattern_data.py: per element and alternative `oracle.match_pattern` in its
float mode, in order.

Sizes 1, 63, 65, 257 and 513: resources 0 and 1 hold 300 and 70 containers, so their segments
straddle waves and workgroups, and the lanes of one wave are decided by different alternatives."""
import json
import os

import numpy as np
import pytest

import foreach_anypattern_data as fad
from kyverno_amd import batch, cli

pytestmark = pytest.mark.gpu
ENGINES = pytest.mark.parametrize("spec", [False, True], ids=["vm", "specialized"])
SIZES = [1, 63, 65, 257, 513]
KV_PATH_NONE = 0xFFFFFFFF
GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "foreach_anypattern.json")))["cases"]
CODE = {"fail": cli.FAIL, "error": cli.ERROR, "skip": cli.SKIP}


@pytest.fixture(scope="module")
def crafted(orc):
    """Policy, resources and expected side of the crafted set at every size (computed once)."""
    pol = fad.crafted_policy()
    sets = {}
    for n in SIZES:
        ress = fad.crafted_resources(n)
        sets[n] = (ress, fad.Expected(orc, pol, ress))
        sets[n][1].check_honest(full=n == 513)
    return pol, sets


def _evaluate(pol, ress, spec, mode=None, device_mask=None, anypattern=True):
    """What cli.evaluate collects, with the result kept (statuses and messages of one kv_validate)."""
    ps = batch.PolicySet([pol], specialize=spec, foreach=True, foreach_pattern=True, foreach_entries=True,
                         foreach_anypattern=anypattern)
    b = batch.Batch(ps, ress)
    kw = {} if mode is None else {"mode": mode}
    r = batch.validate(ps, b, device_mask=device_mask, **kw)
    ev = cli.Evaluation([pol], ress, ps.rules, r.status)
    for ri, res in zip(*np.nonzero(r.status == cli.FAIL)):
        ri, res = int(ri), int(res)
        if ps.rules[ri].foreach:
            ev.foreach_elem[(ri, res)] = r.foreach_element(ri, res)
            if ps.rules[ri].foreach_entries:
                ev.foreach_entry[(ri, res)] = r.foreach_entry(ri, res)
            if cli._any_entry(ev, ps.rules[ri], res):
                ev.foreach_alts[(ri, res)] = cli._foreach_alts(ev, ps.rules[ri], r, res)
    cli.collect_errors(ev, ps, r, ress)
    return ps, b, r, ev


def _diff(names, got, want):
    bad = np.argwhere(got != want)
    return [(names[a], int(b), int(got[a, b]), int(want[a, b])) for a, b in bad[:20]]


def _element(entry, res, idx):
    """Element `idx` of the entry's list on the resource (request.object.<field>[.<field> | [i]]...)."""
    lst = res
    for k in entry["list"].split(".")[2:]:
        if k.endswith("]"):
            k, i = k[:-1].split("[")
            lst = lst[k][int(i)]
        else:
            lst = lst[k]
    return (lst if isinstance(lst, list) else [lst])[idx]


def _check_alternatives(r, rule, res_doc, ri, k, exp):
    """Every alternative of the deciding entry on the deciding element against the model."""
    entry = rule["validate"]["foreach"][exp.entry[(ri, k)]]
    el = _element(entry, res_doc, exp.elem[(ri, k)])
    want = exp.alts[(ri, k)]
    assert len(want) == len(entry["anyPattern"])
    for a, (st, path, text) in enumerate(want):
        assert r.foreach_alt(ri, k, a) == (st, path if st == cli.FAIL else None), (rule["name"], k, a)
        assert r.foreach_alt_error_message(ri, k, a, el) == text, (rule["name"], k, a)
    assert r.foreach_alt(ri, k, len(want)) is None  # (KV_E_RANGE)


# ------------------------------------------------------------------ the hand-derived cases
@ENGINES
@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: c["name"])
def test_golden_cases(spec, case):
    pol, res = case["policy"], case["resource"]
    ps, b, r, ev = _evaluate(pol, [res], spec)
    rule = ps.rules[0]
    n_alt = len(pol["spec"]["rules"][0]["validate"]["foreach"][0]["anyPattern"])
    assert (rule.route, rule.route_reason, rule.foreach, rule.foreach_pattern, rule.foreach_anypattern) == \
        (batch.ROUTE_GPU, "", True, False, n_alt)
    assert batch.STATUS_NAMES[int(r.status[0, 0])] == case["status"]
    assert cli.rule_message(ev, rule, 0) == case["message"]
    assert r.foreach_path(0, 0) is None  # (as for a deny entry)
    if case["status"] == "pass":
        assert r.foreach_element(0, 0) is None and r.foreach_alt(0, 0, 0) is None
    else:
        assert r.foreach_element(0, 0) == case["element"] and r.foreach_entry(0, 0) == 0
        el = res["spec"]["template"]["spec"]["containers"][case["element"]]
        assert r.foreach_error_message(0, 0, el) is None
        for a, want in enumerate(case["alternatives"]):
            st, path = r.foreach_alt(0, 0, a)
            assert (st, path) == (CODE[want["status"]], want.get("path"))
            if "text" in want:
                assert r.foreach_alt_error_message(0, 0, a, el) == want["text"]
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
    assert [x.foreach_anypattern for x in ps.rules] == [fad.n_alternatives(x) for x in rules]
    assert not _diff(names, r.status, exp.status)
    fails = 0
    for ri in range(len(names)):
        for k in range(n):
            assert r.foreach_element(ri, k) == exp.elem.get((ri, k)), (names[ri], k)
            assert r.foreach_entry(ri, k) == exp.entry.get((ri, k)), (names[ri], k)
            assert r.foreach_path(ri, k) is None
            if (ri, k) in exp.alts:
                _check_alternatives(r, rules[ri], ress[k], ri, k, exp)
                fails += 1
            elif fad.on_device(rules[ri]):
                assert r.foreach_alt(ri, k, 0) is None, (names[ri], k)
            if (ri, k) in exp.messages:
                assert cli.rule_message(ev, ps.rules[ri], k) == exp.messages[(ri, k)], (names[ri], k)
            if ps.rules[ri].foreach_anypattern:
                assert r.foreach_message(ri, k) == ("rule skipped" if exp.messages.get((ri, k)) == "rule skipped" else None)
                assert r.deny_message(ri, k) is None
    assert n == 1 or fails
    # kv_result_failures: every FAIL / ERROR / SKIP pair in order, no path id for foreach pairs
    frule, fres, fpid, _ = r.failures()
    want = [(a, c) for a in range(len(names)) for c in range(n) if exp.status[a, c] in (cli.FAIL, cli.ERROR, cli.SKIP)]
    assert list(zip(frule.tolist(), fres.tolist())) == want
    assert all(p == KV_PATH_NONE for p in fpid.tolist())
    assert all(r.path(a, c) is None for a, c in want[:50])


@ENGINES
def test_chain_of_a_deny_entry_and_an_anypattern_entry(crafted, spec):
    """deny-then-any at 513: the deny entry over initContainers decides some pairs (entry 0, no
    alternatives), the anyPattern entry over containers the others (entry 1)."""
    pol, sets = crafted
    ress, exp = sets[513]
    rules = pol["spec"]["rules"]
    ci = [x["name"] for x in rules].index("deny-then-any")
    ps, b, r, ev = _evaluate(pol, ress, spec)
    assert ps.rules[ci].foreach_entries == 2 and ps.rules[ci].foreach_anypattern == 0
    by_entry = {0: 0, 1: 0}
    for k in range(513):
        ent = exp.entry.get((ci, k))
        assert r.foreach_entry(ci, k) == ent, k
        if ent is None:
            continue
        by_entry[ent] += 1
        assert r.foreach_element(ci, k) == exp.elem[(ci, k)], k
        if ent == 0:
            assert (ci, k) not in exp.alts and r.foreach_alt(ci, k, 0) is None
        else:
            _check_alternatives(r, rules[ci], ress[k], ci, k, exp)
        assert cli.rule_message(ev, ps.rules[ci], k) == exp.messages[(ci, k)], k
    assert by_entry[0] and by_entry[1]


@ENGINES
def test_int_typed_values_route_the_element(orc, spec):
    """The guard counts for the alternatives up to and including the first that passes."""
    pol = fad.int_policy()
    for fl in (False, True):
        ress = fad.crafted_resources(257, float_ports=fl)
        exp = fad.Expected(orc, pol, ress)
        ps, b, r, ev = _evaluate(pol, ress, spec)
        assert not _diff(["port-glob-first", "name-first"], r.status, exp.status), fl
        second = exp.status[1][exp.status[1] != cli.NOMATCH]
        if not fl:
            assert (second == cli.PASS).any() and (second == cli.CPU).any()


@ENGINES
def test_counts_and_scopes(crafted, spec):
    pol, sets = crafted
    ress, exp = sets[513]
    ps = batch.PolicySet([pol], specialize=spec, foreach=True, foreach_pattern=True, foreach_entries=True,
                         foreach_anypattern=True)
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
    carries its own key, code-word and record rows."""
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
        if (ri, k) in exp.alts:
            _check_alternatives(r, rules[ri], ress[k], ri, k, exp)
    assert np.array_equal(np.asarray(r.counts).reshape(len(names), -1)[:, :7], exp.counts()[:, :7])


@ENGINES
def test_flag_off_is_cpu(crafted, spec):
    """The same policy compiled without KV_COMPILE_FOREACH_ANYPATTERN: CPU for every matched pair."""
    pol, sets = crafted
    ress, exp = sets[257]
    ps, b, r, ev = _evaluate(pol, ress, spec, anypattern=False)
    want = np.where(exp.status == cli.NOMATCH, cli.NOMATCH, cli.CPU)
    assert np.array_equal(r.status, want)
    assert not any(x.foreach or x.foreach_anypattern for x in ps.rules)
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


def test_apply_command_with_the_flag(tmp_path):
    """`python -m kyverno_amd apply … --device-foreach-anypattern` alone (it implies the pattern and
    foreach flags): the hand-derived FAIL case fails with its message; without the flag the rule is
    routed and nothing fails."""
    import io

    import yaml as _yaml

    case = next(c for c in GOLDEN if c["name"] == "any_fail_condition_anchor_message_with_dot")
    (tmp_path / "p.yaml").write_text(_yaml.safe_dump(case["policy"]))
    (tmp_path / "r.yaml").write_text(_yaml.safe_dump(case["resource"]))
    args = ["apply", str(tmp_path / "p.yaml"), "-r", str(tmp_path / "r.yaml")]
    assert cli.main(args + ["--device-foreach-anypattern"]) == 1
    assert cli.main(args) == 0
    assert cli.main(args + ["--device-foreach-pattern"]) == 0
    out = io.StringIO()  # apply() with the flag alone: evaluate() implies the other two
    rc, _ = cli.apply(args[1:2], args[3:4], foreach_anypattern=True, out=out)
    assert (rc.fail, rc.error) == (1, 0)
    assert f"1. test: {case['message']} \n" in out.getvalue()


@ENGINES
def test_cli_evaluate(crafted, spec):
    """cli.evaluate(foreach_anypattern=True) implies the pattern and foreach flags and composes the
    messages itself."""
    pol, sets = crafted
    ress, exp = sets[65]
    keep = [r for r in pol["spec"]["rules"] if fad.n_alternatives(r)]
    sub = dict(pol, spec={"rules": keep})
    ev = cli.evaluate([sub], ress, specialize=spec, foreach_anypattern=True)
    names = [x["name"] for x in pol["spec"]["rules"]]
    for j, rule in enumerate(ev.rules):
        ri = names.index(rule.name)
        assert np.array_equal(ev.status[j], exp.status[ri]), rule.name
        for k in range(65):
            if (ri, k) in exp.messages:
                assert cli.rule_message(ev, rule, k) == exp.messages[(ri, k)], (rule.name, k)
