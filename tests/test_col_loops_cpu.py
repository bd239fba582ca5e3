"""Per-rule and nested array loops read from path columns (kvjitgen.cpp ColLoop), without a GPU.

The generated kernel of the col_loops_data policies runs on the host under ASan/UBSan
(tests/kvemu.py) over path columns built by the kvcol.h bodies (tools/kvemu/mtab.cpp), with the
generator's cell formats and with every column wide, on the small batch (64 + 7 resources) and on
the whole one (256 + 64 + 5). Statuses against the oracle, and for every pair that fails on
both sides the failing path: the emulator leaves the error record, not the string, so the
record's loop indices must be the array indices of the oracle's path, and within a rule one
pattern node of the records must stand for one path of the oracle with its indices taken out.

The generated source of the benchmarked workload (C2) is checked for the two rules the change
was made for: their programs read no node row.
"""
import json
import os
import re

import numpy as np
import pytest

import col_loops_data as data
import kvemu
from parity_util import oracle_status

WORK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "kvemu_tests")
ENVS = (("narrow", {}), ("wide", {"KVGPU_JIT_NARROW": "0"}))
SIZES = (data.N_SMALL, data.N_RES)


@pytest.fixture(scope="module")
def runs(orc):
    pols, ress = data.policies(), data.resources()
    out = {}
    for tag, env in ENVS:
        work = os.path.join(WORK, "col_loops_" + tag)
        exe = kvemu.build(pols, work, env=env)
        out[tag + "_src"] = open(os.path.join(work, "gen.cpp")).read()
        for n in SIZES:
            out[tag, n] = kvemu.run(exe, b"\n".join(json.dumps(r).encode() for r in ress[:n]), work, env=env)
    out["oracle"] = oracle_status(orc, pols, ress)
    out["paths"] = {(int(rule), int(res)): orc.validate(pols[rule], ress[res])["rules"][0]["path"]
                    for rule, res in np.argwhere(out["oracle"] == 1)}
    return out


def test_inputs_cover_the_cases():
    ress = data.resources()
    assert len(ress) == data.N_RES == 256 + 64 + 5 and data.N_SMALL == 64 + 7
    ports = {}  # (resource, container) -> ports value of the containers that are maps
    for i, r in enumerate(ress):
        for c, ct in enumerate(r["spec"].get("containers", [])):
            if isinstance(ct, dict):
                ports[i, c] = ct.get("ports")
    for first, n in ((0, data.N_SMALL), (0, data.N_RES)):
        vals = [v for (i, _), v in ports.items() if first <= i < n]
        # nested array absent, empty, of 1 and 3 elements, and not an array
        assert None in vals and {len(v) for v in vals if isinstance(v, list)} == {0, 1, 3}
        assert any(isinstance(v, str) for v in vals) and any(isinstance(v, dict) for v in vals)
        # element not a map; leaf absent, null, an array
        elems = [e for v in vals if isinstance(v, list) for e in v]
        assert any(isinstance(e, str) for e in elems)
        leaves = [e.get("containerPort", "absent") for e in elems if isinstance(e, dict)]
        assert "absent" in leaves and None in leaves and any(isinstance(x, list) for x in leaves)
    # a container that is not a map, containers absent and empty
    assert any(isinstance(ct, str) for r in ress[:data.N_SMALL] for ct in r["spec"].get("containers", []))
    assert any("containers" not in r["spec"] for r in ress) and any(r["spec"].get("containers") == [] for r in ress)
    # nested array only in the second / only in the last container, in every wave
    for w in range(0, data.N_RES - 64, 64):
        i = w + data.ONLY_SECOND[0]
        assert [isinstance(ports[i, c], list) for c in range(3)] == [False, True, False]
        i = w + data.ONLY_LAST[0]
        assert [isinstance(ports[i, c], list) for c in range(3)] == [False, False, True]
    # neighbouring lanes differ in nested length: the rows of a parent row are another lane's maximum
    nlen = lambda i, c: len(ports[i, c]) if isinstance(ports.get((i, c)), list) else 0
    for w in range(0, data.N_RES, 64):
        lanes = range(w, min(w + 64, data.N_RES))
        for c in range(2):
            m = max(nlen(i, c) for i in lanes)
            assert m == 3 and sum(nlen(i, c) < m for i in lanes) >= 3
        assert any(nlen(i, 0) != nlen(i + 1, 0) for i in lanes[:-1])
    # the existence anchor: not an array, element not a map, match on the first / last element, none
    for n in SIZES:
        assert {data.volumes_kind(i) for i in range(n)} == set(data.VOLUME_KINDS)


def test_oracle_has_pass_and_fail_on_every_rule(runs):
    ost = runs["oracle"]
    assert ost.shape == (len(data.RULES), data.N_RES)
    for rule in range(ost.shape[0]):
        for n in SIZES:
            assert (ost[rule, :n] == 0).any() and (ost[rule, :n] == 1).any(), (rule, n)
    # failing paths at every depth of the nested loop
    tmpl = {data.path_indices(p)[0] for (rule, _), p in runs["paths"].items() if rule == 0}
    assert tmpl == {"/spec/containers/", "/spec/containers/#/", "/spec/containers/#/ports/", "/spec/containers/#/ports/#/"}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tag", [t for t, _ in ENVS])
def test_statuses_and_failing_paths_match_oracle(runs, tag, n):
    st, rec = runs[tag, n]
    ost = runs["oracle"][:, :n]
    bad = np.argwhere(st != ost)
    assert not len(bad), [(int(a), int(b), int(st[a, b]), int(ost[a, b])) for a, b in bad[:20]]
    tmpl_of = {}  # (several pattern nodes may fail at one path: a missing leaf at its parent's)
    checked = 0
    for rule, res in np.argwhere(ost == 1):
        tmpl, idx = data.path_indices(runs["paths"][int(rule), int(res)])
        r = rec[rule, res]  # ErrRec: kind | flags << 16, pattern node, key node, resource node, idx[4]
        assert list(r[4:4 + len(idx)]) == idx, (int(rule), int(res), tmpl, idx, list(r))
        assert tmpl_of.setdefault((int(rule), int(r[1])), tmpl) == tmpl, (int(rule), int(res), tmpl)
        checked += 1
    assert checked == int((ost == 1).sum()) and checked > 300


def test_loops_read_columns(runs):
    """every array loop of the kernel is a column loop: the ports loops over a nested family"""
    src = runs["narrow_src"]
    body = src[src.index("__global__"):]
    assert "lookup_op(" not in body and not re.search(r"\bN\[c\d", body)
    assert len(re.findall(r"^\s*\{ uint32_t p\d+_c;", body, re.M)) >= 6  # ports x 4 programs, volumes x 2
    from kyverno_amd import batch

    info = kvemu._with_env({"KVGPU_JIT_SKIP_COMPILE": "1"},
                           lambda: batch.PolicySet(data.policies(), specialize=True).jit_info)
    assert info["kernels"] == 1, info


def test_switch_restores_the_walk(tmp_path):
    from kyverno_amd import batch

    src = str(tmp_path / "walk.cpp")
    kvemu._with_env({"KVGPU_JIT_SKIP_COMPILE": "1", "KVGPU_JIT_DUMP": src, "KVGPU_JIT_COLLOOPS": "0"},
                    lambda: batch.PolicySet(data.policies(), specialize=True))
    body = open(src).read()
    body = body[body.index("__global__"):]
    assert "lookup_op(" in body and not re.search(r"\{ uint32_t p\d+_c;", body)


def _rule_text(src, ri):
    """the lines of rule ri's program in the kernel text: from its first label to its last"""
    lines = src[src.index("__global__"):].split("\n")
    at = [k for k, line in enumerate(lines) if re.match(rf"R{ri}_[LS]\d+:;", line)]
    assert at, ri
    return "\n".join(lines[at[0]:at[-1] + 1])


def test_c2_rules_read_no_node_row(tmp_path):
    from kyverno_amd import batch, workloads

    pols = workloads.c2_policies()
    names = [r["name"] for p in pols for r in p["spec"]["rules"]]
    src = str(tmp_path / "c2.cpp")
    kvemu._with_env({"KVGPU_JIT_SKIP_COMPILE": "1", "KVGPU_JIT_DUMP": src},
                    lambda: batch.PolicySet(pols, specialize=True))
    text = open(src).read()
    for name in ("ports-exist", "volumes-any"):
        body = _rule_text(text, names.index(name))
        assert "_c;" in body, name  # (its loop is a column loop)
        assert "N[" not in body and "lookup_op" not in body, name
