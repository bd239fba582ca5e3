"""Narrow path-column cells (kvdevtypes.h ColFmt, kvjitgen.cpp col_plan) without a GPU.

The generated kernels of the narrow_cols_data policies run on the host under ASan/UBSan
(tests/kvemu.py), once with the generator's choice of cell formats and once with every column
wide (KVGPU_JIT_NARROW=0): both must give the oracle's statuses. In the emulator a narrow map
cell stands for a poison node index, so a consumer of a map's index the generator missed reads
out of bounds instead of node 0.
"""
import json
import os

import numpy as np
import pytest

import kvemu
import narrow_cols_data as data
from parity_util import oracle_status

WORK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "kvemu_tests")


def _jit_cols(pols, env):
    from kyverno_amd import batch

    genv = dict(env, KVGPU_JIT_SKIP_COMPILE="1")
    info = kvemu._with_env(genv, lambda: batch.PolicySet(pols, specialize=True).jit_info)
    return info["cols_wide"], info["cols_narrow"]


@pytest.fixture(scope="module")
def runs(orc):
    pols, ress = data.policies(), data.resources()
    blob = b"\n".join(json.dumps(r).encode() for r in ress)
    out = {}
    for tag, env in (("narrow", {}), ("wide", {"KVGPU_JIT_NARROW": "0"})):
        work = os.path.join(WORK, "narrow_cols_" + tag)
        exe = kvemu.build(pols, work, env=env)
        out[tag] = kvemu.run(exe, blob, work, env=env)[0]
    out["oracle"] = oracle_status(orc, pols, ress)
    return out


def test_inputs_cover_the_leaf_kinds():
    ress = data.resources()
    assert len(ress) == data.N_RES == 320
    root = {k: 0 for k in data.LEAF_KINDS}
    elem = {k: 0 for k in data.LEAF_KINDS}
    for i, r in enumerate(ress):
        root[data.root_kind(i)] += 1
        for c in range(data.n_containers(i)):
            elem[data.elem_kind(i, c)] += 1
    assert all(root.values()) and all(elem.values()), (root, elem)
    # the array-at-leaf resources exist (an array of scalars where the pattern has a scalar)
    assert sum(isinstance(r["spec"].get("schedulerName"), list) and len(r["spec"]["schedulerName"]) > 0
               for r in ress) >= 2
    assert sum(isinstance(c.get("imagePullPolicy"), list) and len(c["imagePullPolicy"]) > 0
               for r in ress for c in r["spec"].get("containers", [])) >= 2
    # container counts cycle 0..3 within each 64-resource group: padded element rows are read
    assert [len(r["spec"].get("containers", [])) for r in ress[64:72]] == [0, 1, 2, 3, 0, 1, 2, 3]


def test_generator_picks_both_formats():
    pols = data.policies()
    wide, narrow = _jit_cols(pols, {})
    assert wide >= 1 and narrow >= 1, (wide, narrow)
    wide0, narrow0 = _jit_cols(pols, {"KVGPU_JIT_NARROW": "0"})
    assert narrow0 == 0 and wide0 == wide + narrow


def test_narrow_statuses_match_oracle(runs):
    st, ost = runs["narrow"], runs["oracle"]
    bad = np.argwhere(st != ost)
    assert not len(bad), [(int(a), int(b), int(st[a, b]), int(ost[a, b])) for a, b in bad[:20]]
    for rule in range(st.shape[0]):  # PASS and FAIL both occur on every rule
        assert (st[rule] == 0).any() and (st[rule] == 1).any(), rule


def test_wide_statuses_match_oracle(runs):
    st, ost = runs["wide"], runs["oracle"]
    bad = np.argwhere(st != ost)
    assert not len(bad), [(int(a), int(b), int(st[a, b]), int(ost[a, b])) for a, b in bad[:20]]


def test_narrow_equals_wide(runs):
    assert np.array_equal(runs["narrow"], runs["wide"])
