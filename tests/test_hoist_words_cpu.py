"""Hoist regions of the specialized kernels (kvjitgen.cpp HoistTable::flush) without a GPU.

A region is emitted as its cell loads, then its leaf-word gathers, then one array fix-up. The
generated kernel of the hoist_words_data policy runs on the host under ASan/UBSan
(tests/kvemu.py), with the generator's cell formats and with every column wide
(KVGPU_JIT_NARROW=0): both must give the oracle's statuses over resources that put arrays of
every form at the hoisted leaves, wave by wave (hoist_words_data). The dumped source is checked
for the order of the three parts.

The dumped source (KVGPU_JIT_SKIP_COMPILE) is that of the first plan, which asks for the
three-part layout of every kernel, so this file never runs the first-use-order text that the
build falls back to for a kernel whose registers do not admit the three parts
(kvjitbuild.cpp jit_group_regions). That text is the earlier generator's, run by the GPU suite
wherever a kernel falls back (C4's second kernel, test_gpu_scale.py).
"""
import json
import os
import re

import numpy as np
import pytest

import hoist_words_data as data
import kvemu
from parity_util import oracle_status

WORK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "kvemu_tests")
ENVS = (("narrow", {}), ("wide", {"KVGPU_JIT_NARROW": "0"}))


@pytest.fixture(scope="module")
def runs(orc):
    pols, ress = data.policies(), data.resources()
    blob = b"\n".join(json.dumps(r).encode() for r in ress)
    out = {}
    for tag, env in ENVS:
        work = os.path.join(WORK, "hoist_words_" + tag)
        exe = kvemu.build(pols, work, env=env)
        out[tag] = kvemu.run(exe, blob, work, env=env)[0]
        out[tag + "_src"] = open(os.path.join(work, "gen.cpp")).read()
    out["oracle"] = oracle_status(orc, pols, ress)
    return out


def _array_leaves(i):
    """(region, leaf) of every hoisted leaf of resource i whose value is an array; the region of
    an element leaf is its container"""
    out = [("root", leaf) for leaf in data.ROOT_LEAVES if data.leaf_kind(leaf, i) in data.ARRAY_KINDS]
    out += [(c, leaf) for c in range(data.n_containers(i)) for leaf in data.ELEM_LEAVES
            if data.leaf_kind(leaf, i, c) in data.ARRAY_KINDS]
    return out


def test_inputs_cover_the_waves():
    ress = data.resources()
    assert len(ress) == data.N_RES == 320  # 4 full waves of one workgroup + 1 wave of a partial one
    waves = [[_array_leaves(i) for i in range(w * 64, w * 64 + 64)] for w in range(5)]
    # wave 0: no array at a hoisted leaf
    assert not any(waves[0])
    # waves 1 and 4: a single array lane, at an element leaf / at a root leaf
    assert [l for l, a in enumerate(waves[1]) if a] == [data.W1_LANE] and waves[1][data.W1_LANE] == [(0, "imagePullPolicy")]
    assert [l for l, a in enumerate(waves[4]) if a] == [data.W4_LANE] and waves[4][data.W4_LANE] == [("root", "priorityClassName")]
    # wave 2: several array lanes, one array leaf each, every leaf among them
    lanes2 = [a for a in waves[2] if a]
    assert len(lanes2) >= 6 and all(len(a) == 1 for a in lanes2)
    assert {a[0][1] for a in lanes2} == set(data.LEAVES)
    # wave 3: a lane with two array leaves in one container, and two at the root
    a3 = waves[3][data.W3_LANE]
    assert {(0, "image"), (0, "workingDir"), ("root", "schedulerName"), ("root", "dnsPolicy")} <= set(a3)
    # the arrays: 0, 1, 2 and 3 elements, failing first and last, a null and a nested array element
    arrays = []
    for r in ress:
        vals = [r["spec"].get(leaf) for leaf in data.ROOT_LEAVES]
        vals += [c.get(leaf) for c in r["spec"].get("containers", []) for leaf in data.ELEM_LEAVES]
        arrays += [v for v in vals if isinstance(v, list)]
    assert {len(a) for a in arrays} >= {0, 1, 2, 3}
    assert any(None in a for a in arrays) and any(any(isinstance(e, list) for e in a) for a in arrays)
    bad = {v[1] for v in data.VALUES.values()}
    assert any(len(a) == 3 and a[0] in bad for a in arrays) and any(len(a) == 3 and a[2] in bad for a in arrays)
    # every kind at every leaf; container counts cycle 0..3 within a wave
    for leaf in data.LEAVES:
        kinds = {data.leaf_kind(leaf, i, c) for i in range(data.N_RES)
                 for c in (range(data.n_containers(i)) if leaf in data.ELEM_LEAVES else (0,))}
        assert kinds == set(data.LEAF_KINDS), (leaf, kinds)
    assert [len(r["spec"].get("containers", [])) for r in ress[64:76]] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]


def test_oracle_has_pass_and_fail_on_every_rule(runs):
    ost = runs["oracle"]
    assert ost.shape == (data.N_IMAGE + 6, data.N_RES)
    for rule in range(ost.shape[0]):
        assert (ost[rule] == 0).any() and (ost[rule] == 1).any(), rule


@pytest.mark.parametrize("tag", [t for t, _ in ENVS])
def test_statuses_match_oracle(runs, tag):
    st, ost = runs[tag], runs["oracle"]
    bad = np.argwhere(st != ost)
    assert not len(bad), [(int(a), int(b), int(st[a, b]), int(ost[a, b])) for a, b in bad[:20]]


def test_generator_picks_both_formats():
    from kyverno_amd import batch

    info = kvemu._with_env({"KVGPU_JIT_SKIP_COMPILE": "1"},
                           lambda: batch.PolicySet(data.policies(), specialize=True).jit_info)
    assert info["kernels"] == 1, info
    assert info["cols_wide"] >= 1 and info["cols_narrow"] >= 3, info


def _regions(src):
    """the hoist regions of the kernels' text: the runs of lines that hold a cell load (KVC_LD_),
    a leaf-word gather (KVC_LW_), a fix-up (KVC_LA_), an index select or the fix-up's test, as
    (kind, line) lists"""
    body = src[src.index("__global__"):]
    out, cur = [], []
    for line in body.split("\n"):
        m = re.search(r"\b(KVC_LD_|KVC_LW_|KVC_LA_)", line)
        if m and "#define" not in line:
            cur.append((m.group(1), line))
        elif cur and ("KVC_IX_" in line or "__ballot(" in line or line.strip() == "}"):
            continue
        elif cur:
            out.append(cur)
            cur = []
    return out


@pytest.mark.parametrize("tag", [t for t, _ in ENVS])
def test_regions_load_cells_then_words_then_fix(runs, tag):
    regions = _regions(runs[tag + "_src"])
    assert regions
    for reg in regions:
        kinds = [k for k, _ in reg]
        first_w = kinds.index("KVC_LW_") if "KVC_LW_" in kinds else len(kinds)
        first_a = kinds.index("KVC_LA_") if "KVC_LA_" in kinds else len(kinds)
        # no cell load behind a word gather or a fix-up, no gather behind a fix-up
        assert "KVC_LD_" not in kinds[first_w:], reg
        assert "KVC_LW_" not in kinds[first_a:], reg
        assert kinds.count("KVC_LW_") == kinds.count("KVC_LA_"), reg
    # the loop region of spec.containers: >= 3 leaf cells and >= 4 words, two of them on one cell
    # (the image group's 40 bits); the root region: 3 leaves
    big = max(regions, key=lambda reg: sum(k == "KVC_LW_" for k, _ in reg))
    words = [re.search(r"uint32_t (\w+)_w(\d+) = KVC_LW_", line).groups() for k, line in big if k == "KVC_LW_"]
    assert len(words) >= 4 and len({n for n, _ in words}) >= 3, words
    assert any(sum(n == m for m, _ in words) >= 2 for n, _ in words), words
    assert any(sum(k == "KVC_LW_" for k, _ in reg) == 3 for reg in regions if reg is not big)
