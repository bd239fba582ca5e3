"""`{{element...}}` / `{{request.object...}}` variables in the patterns of validate.foreach entries on
the device (KV_COMPILE_FOREACH_PATVARS: kv_foreach_patv_kernel / kv_foreach_anyv_kernel take the
substitution verdict of the element between the entry gate and the walk, and the walk's dynamic leaf
evaluates the element's substituted value on the batch predicate table; reference
pkg/engine/validation.go:175-202, 549-571), on the bytecode VM and the specialized kernels. The
expected side is the model of tests/foreach_patvars_data.py: the oracle substitutes the pattern in
the element's context and matches the result against the element.

Sizes 1, 63, 65, 257 and 513: resources 0 and 1 hold 300 and 70 containers, so their segments
straddle waves and workgroups; neighbouring lanes hold elements with different outcome ids and
`ports` of 0 to 3 entries."""
import json
import os

import numpy as np
import pytest

import foreach_patvars_data as fvd
from kyverno_amd import batch, cli

pytestmark = pytest.mark.gpu
ENGINES = pytest.mark.parametrize("spec", [False, True], ids=["vm", "specialized"])
SIZES = [1, 63, 65, 257, 513]
KV_PATH_NONE = 0xFFFFFFFF
GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "foreach_patvars.json")))["cases"]


@pytest.fixture(scope="module")
def crafted(orc):
    """Policy, resources and expected side of the crafted set at every size (computed once)."""
    pol = fvd.crafted_policy()
    sets = {}
    for n in SIZES:
        ress = fvd.crafted_resources(n)
        sets[n] = (ress, fvd.Expected(orc, pol, ress))
        sets[n][1].check_honest()
    return pol, sets


def _evaluate(pol, ress, spec, mode=None, device_mask=None, patvars=True):
    """What cli.evaluate collects, with the result kept (statuses and messages of one kv_validate)."""
    ps = batch.PolicySet([pol], specialize=spec, **dict(fvd.ALL, foreach_patvars=patvars))
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
            if cli._pattern_entry(ev, ps.rules[ri], res):
                ev.foreach_path[(ri, res)] = r.foreach_path(ri, res)
            if cli._any_entry(ev, ps.rules[ri], res):
                ev.foreach_alts[(ri, res)] = cli._foreach_alts(ev, ps.rules[ri], r, res)
    cli.collect_errors(ev, ps, r, ress)
    return ps, b, r, ev


def _diff(names, got, want):
    bad = np.argwhere(got != want)
    return [(names[a], int(b), int(got[a, b]), int(want[a, b])) for a, b in bad[:20]]


def _element(entry, res, idx):
    lst = res
    for k in entry["list"].split(".")[2:]:
        lst = lst[k]
    return (lst if isinstance(lst, list) else [lst])[idx]


def _check_pair(r, ev, ps, rules, ress, exp, ri, k):
    """Deciding entry and element, failing path, pattern-error text with the substituted value,
    substitution error and composed message of one pair."""
    key = (ri, k)
    name = rules[ri]["name"]
    assert r.foreach_element(ri, k) == exp.elem.get(key), (name, k)
    assert r.foreach_entry(ri, k) == exp.entry.get(key), (name, k)
    assert r.foreach_subst_error(ri, k) == exp.subst.get(key), (name, k)
    assert r.foreach_path(ri, k) == exp.path.get(key), (name, k)
    if key in exp.err:
        entry = rules[ri]["validate"]["foreach"][exp.entry[key]]
        el = _element(entry, ress[k], exp.elem[key])
        assert r.foreach_error_message(ri, k, el) == exp.err[key], (name, k)
    if key in exp.alts:
        entry = rules[ri]["validate"]["foreach"][exp.entry[key]]
        el = _element(entry, ress[k], exp.elem[key])
        for a, (st, path, text) in enumerate(exp.alts[key]):
            assert r.foreach_alt(ri, k, a) == (st, path if st == cli.FAIL else None), (name, k, a)
            assert r.foreach_alt_error_message(ri, k, a, el) == text, (name, k, a)
    if key in exp.messages:
        assert cli.rule_message(ev, ps.rules[ri], k) == exp.messages[key], (name, k)


# ------------------------------------------------------------------ the reference's test
@ENGINES
def test_reference_fixture(spec):
    case = GOLDEN[0]
    ps, b, r, ev = _evaluate(case["policy"], [case["resource"]], spec)
    rule = ps.rules[0]
    assert (rule.route, rule.route_reason, rule.foreach, rule.foreach_pattern, rule.foreach_patvars) == \
        (batch.ROUTE_GPU, "", True, True, True)
    assert batch.STATUS_NAMES[int(r.status[0, 0])] == case["status"] == "pass"
    assert cli.rule_message(ev, rule, 0) == "rule passed"
    assert r.foreach_element(0, 0) is None and r.foreach_subst_error(0, 0) is None
    assert dict(r.phases).get("foreach", -1.0) >= 0.0
    # a container renamed on one side only is still compared with itself; one without the key is
    # the element's substitution error
    res = json.loads(json.dumps(case["resource"]))
    del res["spec"]["containers"][1]["name"]
    ps, b, r, ev = _evaluate(case["policy"], [res], spec)
    assert int(r.status[0, 0]) == cli.ERROR and r.foreach_element(0, 0) == 1
    want = 'validation failed in foreach rule for variable substitution failed: Unknown key "name" in path'
    assert r.foreach_subst_error(0, 0) == want == cli.rule_message(ev, ps.rules[0], 0)
    assert r.foreach_error_message(0, 0, res["spec"]["containers"][1]) is None


# ------------------------------------------------------------------ crafted parity
@ENGINES
@pytest.mark.parametrize("n", SIZES)
def test_crafted_parity(crafted, spec, n):
    pol, sets = crafted
    ress, exp = sets[n]
    rules = pol["spec"]["rules"]
    names = [x["name"] for x in rules]
    ps, b, r, ev = _evaluate(pol, ress, spec)
    assert [x.foreach_patvars for x in ps.rules] == [fvd.rule_has_variables(x) for x in rules]
    assert not _diff(names, r.status, exp.status)
    for ri in range(len(names)):
        for k in range(n):
            _check_pair(r, ev, ps, rules, ress, exp, ri, k)
            if ps.rules[ri].foreach:
                assert r.deny_message(ri, k) is None
    assert n == 1 or (exp.subst and exp.err and exp.path and exp.alts)
    # a FAIL at a dynamic leaf names the substituted value
    if n >= 63:
        ai = names.index("name-is-alias")
        texts = [exp.err[(ri, k)] for (ri, k) in exp.path if ri == ai]
        assert texts and all("does not match 'xc" in t for t in texts), texts[:3]
    # kv_result_failures: every FAIL / ERROR / SKIP pair in order, no path id for foreach pairs
    frule, fres, fpid, _ = r.failures()
    want = [(a, c) for a in range(len(names)) for c in range(n) if exp.status[a, c] in (cli.FAIL, cli.ERROR, cli.SKIP)]
    assert list(zip(frule.tolist(), fres.tolist())) == want
    assert all(p == KV_PATH_NONE for p in fpid.tolist())


@ENGINES
def test_anypattern_composition(crafted, spec):
    """any-c0-or-alias at 513: a c0 element without `alias` is ERROR although alternative 0 matches
    it (the whole list is substituted first); FAIL pairs carry both alternatives' outcomes."""
    pol, sets = crafted
    ress, exp = sets[513]
    rules = pol["spec"]["rules"]
    ai = [x["name"] for x in rules].index("any-c0-or-alias")
    ps, b, r, ev = _evaluate(pol, ress, spec)
    assert ps.rules[ai].foreach_anypattern == 2 and ps.rules[ai].foreach_patvars
    seen = {"subst": 0, "alts": 0, "c0": 0}
    for k in range(513):
        assert int(r.status[ai, k]) == exp.status[ai, k], k
        _check_pair(r, ev, ps, rules, ress, exp, ai, k)
        if (ai, k) in exp.subst:
            seen["subst"] += 1
            el = _element(rules[ai]["validate"]["foreach"][0], ress[k], exp.elem[(ai, k)])
            seen["c0"] += el["name"] == "c0"
        seen["alts"] += (ai, k) in exp.alts
    assert seen["subst"] and seen["alts"] and seen["c0"], seen


@ENGINES
def test_entries_composition(crafted, spec):
    """deny-then-leaked at 513: the pattern of the second entry reads `mark`, a key of the last
    initContainer only; with initContainers it resolves through the leak, without them every element
    fails the substitution."""
    pol, sets = crafted
    ress, exp = sets[513]
    rules = pol["spec"]["rules"]
    ci = [x["name"] for x in rules].index("deny-then-leaked")
    ps, b, r, ev = _evaluate(pol, ress, spec)
    assert ps.rules[ci].foreach_entries == 2 and ps.rules[ci].foreach_patvars
    got = {cli.PASS: 0, cli.FAIL: 0, cli.ERROR: 0}
    for k in range(513):
        st = int(r.status[ci, k])
        assert st == exp.status[ci, k], k
        _check_pair(r, ev, ps, rules, ress, exp, ci, k)
        if st in got:
            got[st] += 1
            init = "initContainers" in ress[k]["spec"]
            assert (st == cli.ERROR) == (not init), k
            if st == cli.ERROR:
                assert exp.subst[(ci, k)].endswith('Unknown key "mark" in path') and exp.entry[(ci, k)] == 1
    assert all(got.values()), got


@ENGINES
def test_int_under_a_substituted_glob(orc, spec):
    """A substituted "?0" over an int-typed port is CPU; over a float port it is evaluated."""
    pol = fvd.int_policy()
    for fl in (False, True):
        ress = fvd.crafted_resources(257, float_ports=fl)
        exp = fvd.Expected(orc, pol, ress)
        ps, b, r, ev = _evaluate(pol, ress, spec)
        assert not _diff(["port-glob", "name-set"], r.status, exp.status), fl
        first = exp.status[0][exp.status[0] != cli.NOMATCH]
        if fl:
            assert (first == cli.FAIL).any() and (first == cli.CPU).sum() * 5 < len(first)
        else:
            assert set(first.tolist()) <= {cli.CPU, cli.SKIP}


@ENGINES
def test_counts_and_scopes(crafted, spec):
    pol, sets = crafted
    ress, exp = sets[513]
    ps = batch.PolicySet([pol], specialize=spec, **fvd.ALL)
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
    """The 513 set as three logical parts of one device: each part resolves, uploads and walks its
    own elements and carries its own key and record rows."""
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
    for (ri, k) in exp.elem:
        _check_pair(r, ev, ps, rules, ress, exp, ri, k)
    assert np.array_equal(np.asarray(r.counts).reshape(len(names), -1)[:, :7], exp.counts()[:, :7])


@ENGINES
def test_flag_off_is_cpu(crafted, spec):
    """The rules with variable strings compiled without KV_COMPILE_FOREACH_PATVARS: CPU for every
    matched pair, and no foreach phase."""
    pol, sets = crafted
    ress, exp = sets[257]
    keep = [x for x in pol["spec"]["rules"] if fvd.rule_has_variables(x) or not fvd.on_device(x)]
    sub = dict(pol, spec={"rules": keep})
    names = [x["name"] for x in pol["spec"]["rules"]]
    ps, b, r, ev = _evaluate(sub, ress, spec, patvars=False)
    rows = [names.index(x["name"]) for x in keep]
    want = np.where(exp.status[rows] == cli.NOMATCH, cli.NOMATCH, cli.CPU)
    assert np.array_equal(r.status, want)
    assert not any(x.foreach or x.foreach_patvars for x in ps.rules)
    assert all(x.route_reason == "foreach" for x in ps.rules)
    assert "foreach" not in dict(r.phases)


def test_apply_command_with_the_flag(tmp_path):
    """`python -m kyverno_amd apply … --device-foreach-patvars` alone (it implies the pattern and
    foreach flags): the reference's Pod passes, a Pod with a container without `name` is an error;
    without the flag the rule is routed and nothing fails."""
    import yaml as _yaml

    case = GOLDEN[0]
    bad = json.loads(json.dumps(case["resource"]))
    del bad["spec"]["containers"][0]["name"]
    (tmp_path / "p.yaml").write_text(_yaml.safe_dump(case["policy"]))
    (tmp_path / "r.yaml").write_text(_yaml.safe_dump(case["resource"]))
    (tmp_path / "b.yaml").write_text(_yaml.safe_dump(bad))
    good_args = ["apply", str(tmp_path / "p.yaml"), "-r", str(tmp_path / "r.yaml")]
    bad_args = ["apply", str(tmp_path / "p.yaml"), "-r", str(tmp_path / "b.yaml")]
    assert cli.main(good_args + ["--device-foreach-patvars"]) == 0
    assert cli.main(bad_args + ["--device-foreach-patvars"]) == 1
    assert cli.main(bad_args) == 0
    assert cli.main(bad_args + ["--device-foreach-pattern"]) == 0
    ev = cli.evaluate([case["policy"]], [bad], foreach_patvars=True)
    assert int(ev.status[0, 0]) == cli.ERROR
    assert cli.rule_message(ev, ev.rules[0], 0).endswith('variable substitution failed: Unknown key "name" in path')
