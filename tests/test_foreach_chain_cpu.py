"""validate.foreach rules of several entries on the device, without a GPU
(KV_COMPILE_FOREACH_ENTRIES: kvcond.cpp compile_foreach, kvvars.cpp resolve_elem_overlay,
kvforeach.h kv_fe_chain; reference pkg/engine/validation.go:204-283 and the JSON context's
Checkpoint / Reset): the chain model against the golden cases (tests/golden/foreach_chain.json),
routing under every flag combination, the interning of chains, sets and leak contexts, tables that
do not change where no rule has several entries, the host fold (`kv_batch_foreach_chain_fold`, the
twin of the entry kernels and kv_foreach_chain_kernel) and the emulator against the model, shards
against the whole, and the message side (`cli.foreach_leak_base`).

Messages without a GPU: the FAIL text of a pair a deny entry decided is composed by
cli.rule_message from the host fold's entry and element; the ERROR and SKIP texts come from
kv_batch_foreach_chain_message, the host side of kv_result_foreach_message. The elements of a
pattern entry are walked on the device only (no host evaluator), so the texts of the two chains
with a pattern entry are compared in tests/test_gpu_foreach_chain.py alone."""
import copy
import json
import os

import numpy as np
import pytest

import foreach_chain_data as cd
import foreach_chain_model
import foreach_data as fd
from kyverno_amd import _native, batch, cli, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 65, 257]
ALL = {"foreach": True, "foreach_pattern": True, "foreach_entries": True}


@pytest.fixture(scope="module")
def expected(orc):
    """The expected side of the crafted set at every size (computed once, shared)."""
    pol = cd.crafted_policy()
    return pol, {n: cd.Expected(orc, pol, cd.crafted_resources(n)) for n in SIZES}


# ------------------------------------------------------------------ the model, pinned
def test_golden_fixture_shape():
    first = cd.CASES_GOLDEN[0]
    assert first["name"] == "Test_foreach_skip_initContainer_pass" and first["origin"] == "transcribed"
    assert first["src"] == "pkg/engine/validation_test.go:2937-2990" and first["device"] == {"route": "cpu", "reason": "foreach"}
    assert ".." in first["policy"]["spec"]["rules"][0]["validate"]["foreach"][1]["list"]
    derived = [c for c in cd.CASES_GOLDEN if c["origin"] == "derived"]
    assert len(derived) >= 4 and all(c["device"] == {"route": "gpu", "reason": ""} for c in derived)
    assert all(c["resource"] == first["resource"] for c in derived)
    assert derived[0]["policy"]["spec"]["rules"][0]["validate"]["foreach"][1]["list"] == \
        first["policy"]["spec"]["rules"][0]["validate"]["foreach"][1]["list"].replace("..", ".")


@pytest.mark.parametrize("case", [c for c in cd.CASES_GOLDEN if c["origin"] == "derived"], ids=lambda c: c["name"])
def test_model_matches_derived_cases(orc, case):
    m = foreach_chain_model.Model(orc)
    st, en, el, msgs, _ = m.chain(case["policy"]["spec"]["rules"][0], case["resource"])
    assert (st, en, el, msgs) == (case["status"], case["entry"], case["element"], [case["message"]])


def test_merge():
    m = foreach_chain_model.merge
    base = {"a": 1, "sc": {"caps": {"drop": ["ALL"]}, "priv": False}, "args": ["a", "b"]}
    assert m(base, {"sc": {"priv": True}, "args": ["x"], "b": 2}) == \
        {"a": 1, "sc": {"caps": {"drop": ["ALL"]}, "priv": True}, "args": ["x"], "b": 2}
    assert m(base, {"sc": "none"})["sc"] == "none" and m({"sc": "none"}, {"sc": {"x": 1}})["sc"] == {"x": 1}
    assert cli.merge_maps(base, {"sc": {"priv": True}, "args": ["x"]}) == m(base, {"sc": {"priv": True}, "args": ["x"]})


@pytest.mark.parametrize("case", cd.CASES_GOLDEN, ids=lambda c: c["name"])
def test_golden_routes(case):
    """The reference's own case has `..` in its second list: routed with every flag on; the derived
    ones are device rules with the flags and routed without the new one."""
    on = batch.PolicySet([case["policy"]], **ALL).rules[0]
    off = batch.PolicySet([case["policy"]], foreach=True, foreach_pattern=True).rules[0]
    want = (batch.ROUTE_CPU if case["device"]["route"] == "cpu" else batch.ROUTE_GPU, case["device"]["reason"])
    assert (on.route, on.route_reason) == want and on.foreach == (want[0] == batch.ROUTE_GPU)
    assert on.foreach_entries == (2 if want[0] == batch.ROUTE_GPU else 0)
    assert (off.route, off.route_reason, off.foreach, off.foreach_entries) == (batch.ROUTE_CPU, "foreach", False, 0)


@pytest.mark.parametrize("case", [c for c in cd.CASES_GOLDEN if c["origin"] == "derived"], ids=lambda c: c["name"])
def test_host_fold_derived_cases(case):
    ps = batch.PolicySet([case["policy"]], **ALL)
    st, en, el = ps.foreach_chain_fold(batch.Batch(ps, [case["resource"]]))
    entries = case["policy"]["spec"]["rules"][0]["validate"]["foreach"]
    if any("pattern" in e for e in entries):
        assert st[0, 0] == 255  # (no host evaluator for a pattern set)
        return
    assert batch.STATUS_NAMES[st[0, 0]] == case["status"]
    assert en[0, 0] == (cd.NONE if case["entry"] is None else case["entry"])
    assert el[0, 0] == (cd.NONE if case["element"] is None else case["element"])


# ------------------------------------------------------------------ routing
DENY = {"list": cd.C, "deny": {"conditions": [{"key": "{{element.image}}", "operator": "Equals", "value": "x"}]}}
DENY_I = dict(DENY, list=cd.I)
PAT = {"list": cd.I, "pattern": {"name": "i*"}}
PRE = {"all": [{"key": "{{request.object.metadata.labels.tier}}", "operator": "Equals", "value": "web"}]}
PRE_OUT = {"all": [{"key": "{{request.operation}}", "operator": "Equals", "value": "CREATE"}]}


def _routing_policy():
    def rule(name, entries, **more):
        return {"name": name, "match": cd.POD, "validate": {"message": "m", "foreach": copy.deepcopy(entries)}, **more}
    return fd.pd._policy("foreach-chain-routing", [
        rule("one", [DENY]),
        rule("two-deny", [DENY, DENY_I]),
        rule("deny-pattern", [DENY, PAT]),
        rule("pattern-deny", [PAT, DENY]),
        rule("sixteen", [DENY] * 16),
        rule("seventeen", [DENY] * 17),
        rule("any-pattern-entry", [DENY, {"list": cd.I, "anyPattern": [{"name": "i*"}]}]),
        rule("context-entry", [DENY, dict(DENY_I, context=[{"name": "cm", "configMap": {"name": "a", "namespace": "b"}}])]),
        rule("old-list-preconditions", [DENY, dict(DENY_I, preconditions=[{"key": "{{element.name}}", "operator": "Equals", "value": "c"}])]),
        rule("list-out", [DENY, dict(DENY_I, list="request.object.spec.containers[*]")]),
        rule("rule-context", [DENY, DENY_I], context=[{"name": "cm", "configMap": {"name": "a", "namespace": "b"}}]),
        rule("behind-preconditions", [DENY, DENY_I], preconditions=PRE),
        rule("preconditions-out", [DENY, DENY_I], preconditions=PRE_OUT),
    ])


GPU, ROUTED = (batch.ROUTE_GPU, ""), (batch.ROUTE_CPU, "foreach")


@pytest.mark.parametrize("flags,want", [
    ({}, {}),
    ({"foreach": True}, {"one": 1}),
    ({"foreach": True, "foreach_pattern": True}, {"one": 1}),
    ({"foreach": True, "foreach_entries": True},
     {"one": 1, "two-deny": 2, "sixteen": 16, "behind-preconditions": 2}),
    (ALL, {"one": 1, "two-deny": 2, "deny-pattern": 2, "pattern-deny": 2, "sixteen": 16, "behind-preconditions": 2}),
], ids=["none", "foreach", "pattern", "entries", "all"])
def test_routing(flags, want):
    """Every flag combination: which rules are device rules (name -> entries), kv_rule_info and the
    per-rule accessors. Everything else keeps (CPU, "foreach"), `preconditions-out` (CPU,
    "preconditions") where its entries are in scope."""
    ps = batch.PolicySet([_routing_policy()], **flags)
    info, chains = ps.foreach_info, ps.foreach_chain_info
    for r in ps.rules:
        n = want.get(r.name, 0)
        if r.name == "preconditions-out" and "two-deny" in want:
            assert (r.route, r.route_reason) == (batch.ROUTE_CPU, "preconditions"), r.name
        else:
            assert (r.route, r.route_reason) == (GPU if n else ROUTED), (r.name, r.route_reason)
        assert r.foreach == bool(n) and r.foreach_entries == (n if n > 1 else 0), r.name
        assert not r.foreach_pattern and not r.deny  # (kv_rule_foreach_pattern / _deny_set stay 0 for a chain rule)
        # kv_rule_foreach_set (and kv_rule_info.foreach_set) stay 0 for a chain rule
        assert (info["rule_sets"][r.index] > 0) == (n == 1), r.name
        assert (chains["rule_chains"][r.index] > 0) == (n > 1), r.name
    if not flags.get("foreach_entries"):
        assert chains["chains"] == 0


def test_flag_needs_foreach():
    lib = _native.lib()
    data = json.dumps([_routing_policy()]).encode()
    for flags in (batch.COMPILE_FOREACH_ENTRIES, batch.COMPILE_FOREACH_ENTRIES | batch.COMPILE_DENY,
                  batch.COMPILE_FOREACH_ENTRIES | batch.COMPILE_SPECIALIZE):
        h, err = _native.ctypes.c_void_p(), _native.new_err()
        assert lib.kv_compile(data, len(data), flags, _native.ctypes.byref(h), _native.ctypes.byref(err)) == -1
    with pytest.raises(Exception):
        batch.PolicySet([_routing_policy()], foreach_entries=True)


def test_rollback_leaves_nothing_behind():
    """A rule whose last entry is outside the scope: the tables are those of the set without it."""
    rules = _routing_policy()["spec"]["rules"]
    keep = [r for r in rules if r["name"] in ("one", "two-deny")]
    out = [r for r in rules if r["name"] in ("any-pattern-entry", "context-entry", "old-list-preconditions", "list-out",
                                             "seventeen")]
    extra = {"name": "pattern-then-out", "match": cd.POD, "validate": {"message": "m", "foreach": [
        {"list": cd.E, "pattern": {"name": "d*"}}, {"list": cd.I, "deny": {"conditions": [
            {"key": "{{element.stage}}", "operator": "Equals", "value": "x"}]}}, {"list": cd.C, "anyPattern": [{}]}]}}
    pa, pb = fd.pd._policy("p", keep), fd.pd._policy("p", [keep[0]] + out + [extra] + [keep[1]])
    a = batch.PolicySet([pa], **ALL)
    b = batch.PolicySet([pb], **ALL)
    ia, ib = a.foreach_info, b.foreach_info
    assert {k: ia[k] for k in ("sets", "lists", "conditions", "strings")} == \
        {k: ib[k] for k in ("sets", "lists", "conditions", "strings")} == {"sets": 2, "lists": 2, "conditions": 2, "strings": 2}
    assert a.foreach_chain_info["chain_sets"] == b.foreach_chain_info["chain_sets"] == [[0, 1]]
    # the per-batch tables (strings, columns, planes, contexts' rows, pattern and chain tables) byte for byte
    ress = cd.crafted_resources(65)
    assert a.foreach_tables(batch.Batch(a, ress)) == b.foreach_tables(batch.Batch(b, ress))


def test_rollback_leaves_no_program_behind(tmp_path):
    """A pattern entry compiled before the entry that routes its rule: the instructions, pattern
    nodes and slot fix-ups of its program are taken back. The generated source of the set with the
    routed rule is that of the set with the same rule routed at its first entry (where nothing is
    compiled at all)."""
    def pol(first):
        return fd.pd._policy("p", [
            {"name": "one", "match": cd.POD, "validate": {"message": "m", "foreach": [copy.deepcopy(DENY)]}},
            {"name": "routed", "match": cd.POD, "validate": {"message": "m", "foreach": first + [
                {"list": cd.C, "pattern": {"image": "!*:latest", "=(ports)": [{"containerPort": "<1024"}]}},
                {"list": cd.I, "anyPattern": [{}]}]}},
            {"name": "plain", "match": cd.POD, "validate": {"message": "m", "pattern": {"spec": {"containers": [{"image": "?*"}]}}}},
            {"name": "pat", "match": cd.POD, "validate": {"message": "m", "foreach": [{"list": cd.C, "pattern": {"image": "?*"}}]}},
        ])
    late, _ = _dump([pol([])], str(tmp_path), "late.cpp", **ALL)  # routed at its second entry, after a pattern compiled
    early, _ = _dump([pol([{"list": cd.C, "anyPattern": [{}]}])], str(tmp_path), "early.cpp", **ALL)  # routed at its first
    assert len(late) > 10000 and late == early


# ------------------------------------------------------------------ interning
def test_interning(expected):
    pol = expected[0]
    ps = batch.PolicySet([pol], **ALL)
    names = [r["name"] for r in pol["spec"]["rules"]]
    info, ch = ps.foreach_info, ps.foreach_chain_info
    chain_of = lambda n: ch["chain_sets"][ch["rule_chains"][names.index(n)] - 1]  # noqa: E731
    # a position-1 entry shares the single-entry rule's set
    assert chain_of("pull-policy")[0] == info["rule_sets"][names.index("single-pull")] - 1
    # the same entry at position 2 after another list: another leak context, another set
    assert chain_of("pull-policy")[1] != chain_of("pull-policy-after-ephemeral")[1]
    # the same chain three times
    assert ch["rule_chains"][names.index("pull-policy")] == ch["rule_chains"][names.index("shared")] == \
        ch["rule_chains"][names.index("behind-preconditions")] > 0
    # the always-passing first entry is one set, whatever follows it
    firsts = {chain_of(n)[0] for n in ("gated-pull", "nested-merge", "array-replaced", "three-entries", "pattern-raw")}
    assert len(firsts) == 1
    assert len(chain_of("three-entries")) == 3 and ch["chains"] == 9 and info["lists"] == 3
    # an entry without an `element` string keeps the first entry's context: the pattern entry of
    # `deny-pattern` (position 2) is the set of the same entry at position 1
    rp = batch.PolicySet([_routing_policy()], **ALL)
    rn = [r.name for r in rp.rules]
    rc = rp.foreach_chain_info
    assert rc["chain_sets"][rc["rule_chains"][rn.index("deny-pattern")] - 1][1] == \
        rc["chain_sets"][rc["rule_chains"][rn.index("pattern-deny")] - 1][0]
    # ... and a deny entry with an element string does not: DENY after the pattern entry's list
    assert rc["chain_sets"][rc["rule_chains"][rn.index("pattern-deny")] - 1][1] != \
        rc["chain_sets"][rc["rule_chains"][rn.index("deny-pattern")] - 1][0]


def _dump(pols, tmp, name, **flags):
    path = os.path.join(tmp, name)
    old = {k: os.environ.get(k) for k in ("KVGPU_JIT_DUMP", "KVGPU_JIT_SKIP_COMPILE")}
    os.environ.update(KVGPU_JIT_DUMP=path, KVGPU_JIT_SKIP_COMPILE="1")
    try:
        ps = batch.PolicySet(pols, specialize=True, **flags)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return open(path, "rb").read(), ps


def test_policy_sets_without_chains_are_unchanged(tmp_path):
    """foreach_data's policy (its `two-entries` rule aside, which the flag takes) without that rule,
    and the C2 twins: the generated source, the foreach tables and the host fold are the same with
    and without the new flag."""
    pol = fd.crafted_policy()
    pol["spec"]["rules"] = [r for r in pol["spec"]["rules"] if r["name"] != "two-entries"]
    ress = fd.crafted_resources(65)
    for name, pols in (("crafted", [pol]), ("c2", workloads.c2_policies()), ("c2-foreach", workloads.c2_foreach_policies())):
        a, pa = _dump(pols, str(tmp_path), name + "-off.cpp", foreach=True)
        b, pb = _dump(pols, str(tmp_path), name + "-on.cpp", foreach=True, foreach_entries=True)
        assert len(a) > 10000 and a == b, name
        assert pa.foreach_info == pb.foreach_info and pb.foreach_chain_info["chains"] == 0
        if name != "c2":  # the foreach tables of a batch, byte for byte
            rs = ress if name == "crafted" else batch.synth(workloads.SEED, 300)
            ta, tb = pa.foreach_tables(batch.Batch(pa, rs)), pb.foreach_tables(batch.Batch(pb, rs))
            assert len(ta) > 1000 and ta == tb, name
    # the full policy under the existing flags keeps `two-entries` routed (the existing tests pin it)
    full = batch.PolicySet([fd.crafted_policy()], foreach=True)
    assert {r.name: r.route_reason for r in full.rules}["two-entries"] == "foreach"


def test_exported_symbols():
    lib = _native.lib()
    for s in ("kv_policyset_foreach_chains", "kv_rule_foreach_chain", "kv_chain_entry_set", "kv_batch_foreach_chain_fold",
              "kv_result_foreach_entry", "kv_batch_foreach_chain_message", "kv_foreach_set_pattern", "kv_batch_foreach_tables"):
        assert s in _native.EXPORTED_SYMBOLS and getattr(lib, s) is not None
    hdr = open(os.path.join(ROOT, "include", "kvgpu.h")).read()
    assert "KV_COMPILE_FOREACH_ENTRIES = 16" in hdr and batch.COMPILE_FOREACH_ENTRIES == 16
    assert "int kv_rule_foreach_chain(const kv_policyset* ps, uint32_t rule, uint32_t* chain_plus_1, uint32_t* n_entries);" in hdr
    assert "int kv_result_foreach_entry(const kv_result* r, uint32_t rule, uint64_t res, uint32_t* entry);" in hdr


def test_workload_twin():
    pols = workloads.c2_foreach_chain_policies()
    assert len(pols[0]["spec"]["rules"]) == 100
    ps = batch.PolicySet(pols, foreach=True, foreach_entries=True)
    assert all(r.route == batch.ROUTE_GPU and r.foreach_entries == 2 for r in ps.rules)
    assert ps.foreach_chain_info["chains"] == 8 and ps.foreach_info["lists"] == 2
    assert all((r.route, r.route_reason) == ROUTED for r in batch.PolicySet(pols, foreach=True).rules)


# ------------------------------------------------------------------ the host fold and the emulator
def test_check_cases(expected):
    expected[1][257].check_cases()


@pytest.mark.parametrize("n", SIZES)
def test_host_fold_matches_model(expected, n):
    """kv_batch_foreach_chain_fold per chain against the model alone, in caller order: the status
    of every resource, the deciding entry and element of every FAIL / ERROR one; then the message
    of every FAIL / ERROR / SKIP pair the fold decides: FAIL through cli.rule_message (the message
    sees the element over the leak base), ERROR (the first string unresolved on the overlay) and
    SKIP through kv_batch_foreach_chain_message."""
    pol, exp = expected[0], expected[1][n]
    ps = batch.PolicySet([pol], **ALL)
    b = batch.Batch(ps, exp.resources)
    st, en, el = ps.foreach_chain_fold(b)
    chains = ps.foreach_chain_info["rule_chains"]
    ev = cli.Evaluation([pol], exp.resources, ps.rules, exp.status)
    bad, compared = [], 0
    for ri, rule in enumerate(pol["spec"]["rules"]):
        if not (cd.on_device(rule) and cd.is_chain(rule)):
            assert chains[ri] == 0
            continue
        c = chains[ri] - 1
        if rule["name"] in cd.PATTERN_RULES:
            assert (st[c] == 255).all()
            continue
        for k in range(n):
            want = int(exp.fold[ri, k])
            if int(st[c, k]) != want:
                bad.append((rule["name"], k, int(st[c, k]), want))
            elif want in (cd.FAIL, cd.ERROR) and (int(en[c, k]), int(el[c, k])) != (int(exp.fold_entry[ri, k]), int(exp.fold_elem[ri, k])):
                bad.append((rule["name"], k, (int(en[c, k]), int(el[c, k])), (int(exp.fold_entry[ri, k]), int(exp.fold_elem[ri, k]))))
    assert not bad, bad[:20]
    kinds = set()
    for ri, rule in enumerate(pol["spec"]["rules"]):
        if not (cd.on_device(rule) and cd.is_chain(rule)) or rule["name"] in cd.PATTERN_RULES:
            continue
        c = chains[ri] - 1
        for k in range(n):
            want, got = int(exp.fold[ri, k]), ps.foreach_chain_message(b, c, k)
            # the fold's own text, whatever match and the rule's preconditions do to the pair
            if want == cd.SKIP:
                assert got == "rule skipped", (rule["name"], k)
            elif want != cd.ERROR:
                assert got is None, (rule["name"], k)
            msgs = exp.messages.get((ri, k))
            if msgs is None or exp.gated[ri, k] or exp.status[ri, k] not in (cd.FAIL, cd.ERROR, cd.SKIP):
                if want == cd.ERROR:
                    assert got is not None and got.startswith(foreach_chain_model.HEAD), (rule["name"], k)
                continue
            if exp.status[ri, k] == cd.FAIL:
                ev.foreach_entry[(ri, k)], ev.foreach_elem[(ri, k)] = int(en[c, k]), int(el[c, k])
                got = cli.rule_message(ev, ps.rules[ri], k)
            assert (got == msgs[0]) if len(msgs) == 1 else (got in msgs), (rule["name"], k, got, msgs)
            kinds.add(int(exp.status[ri, k]))
            compared += 1
    assert compared or n == 1
    if n == 257:
        assert kinds == {cd.FAIL, cd.ERROR, cd.SKIP}


@pytest.mark.parametrize("n", SIZES)
def test_chains_on_the_emulator(expected, n):
    """The crafted set through the host build of the generated kernels: the driver fills the entry
    sets' rows, then the chains' rows through kv_fe_chain; every status against the decomposition.
    At 257 also as three shards (of 64-resource groups) against the whole."""
    import kvemu_chain

    pol, exp = expected[0], expected[1][n]
    work = os.path.join(ROOT, "build", "kvemu_tests", f"foreach_chain_{n}")
    exe = kvemu_chain.build([pol], work)
    data = b"\n".join(json.dumps(r).encode() for r in exp.resources)
    st = kvemu_chain.run(exe, data, work)
    bad = np.argwhere(st != exp.status)
    assert not len(bad), [(pol["spec"]["rules"][a]["name"], int(b), int(st[a, b]), int(exp.status[a, b])) for a, b in bad[:20]]
    if n == 257:
        assert np.array_equal(kvemu_chain.run(exe, data, work, env={"KVEMU_SHARDS": "3"}), st)


def test_merged_batches_carry_overlay_rows():
    """The threaded ingest (parts merged, outcome ids re-interned) gives the fold of the serial one."""
    pol = cd.crafted_policy()
    data = "\n".join(json.dumps(r) for r in cd.crafted_resources(900)).encode()
    assert len(data) >= 1 << 20  # (below that the ingest is serial)
    ps = batch.PolicySet([pol], **ALL)
    got = []
    for t in ("1", "4"):
        os.environ["KVGPU_INGEST_THREADS"] = t
        try:
            got.append(ps.foreach_chain_fold(batch.Batch(ps, data)))
        finally:
            os.environ.pop("KVGPU_INGEST_THREADS", None)
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b)
    assert len({int(x) for x in np.unique(got[0][0])}) >= 5


def test_fold_range_checks():
    ps = batch.PolicySet([cd.crafted_policy()], **ALL)
    b = batch.Batch(ps, cd.crafted_resources(3))
    out = np.zeros(3, dtype=np.uint8)
    lib = _native.lib()
    n = ps.foreach_chain_info["chains"]
    assert lib.kv_batch_foreach_chain_fold(ps._h, b._h, n, out.ctypes.data, None, None, 3) == -4
    assert lib.kv_batch_foreach_chain_fold(ps._h, b._h, 0, out.ctypes.data, None, None, 2) == -4
    assert lib.kv_batch_foreach_chain_fold(ps._h, b._h, 0, out.ctypes.data, None, None, 3) == 0
    names = [r.name for r in ps.rules]
    mixed = ps.foreach_chain_info["rule_chains"][names.index("mixed")] - 1
    assert lib.kv_batch_foreach_chain_fold(ps._h, b._h, mixed, out.ctypes.data, None, None, 3) == -1
    s = _native.ctypes.c_uint32()
    assert lib.kv_chain_entry_set(ps._h, 0, 2, _native.ctypes.byref(s)) == -4


# ------------------------------------------------------------------ messages
def test_foreach_leak_base():
    res = {"spec": {"containers": [{"name": "c0", "sc": {"caps": "x"}}, {"name": "c1", "pull": "Always", "sc": {"priv": False}}],
                    "initContainers": [], "one": {"name": "solo", "sc": {"priv": True}}}}
    ents = [{"list": "request.object.spec.containers"}, {"list": "request.object.spec.missing"},
            {"list": "request.object.spec.initContainers"}, {"list": "request.object.spec.one"}, {"list": "x"}]
    base = cli.foreach_leak_base
    assert base(ents, res, 0) is None
    assert base(ents, res, 1) == base(ents, res, 2) == base(ents, res, 3) == res["spec"]["containers"][1]
    assert base(ents, res, 4) == {"name": "solo", "pull": "Always", "sc": {"priv": True}}
    assert base(ents[1:3], res, 2) is None
