"""Hoist regions on the device: the hoist_words_data policies (a 40-member image group whose cell
needs two table words, element and root leaves sharing their regions, one wide column) over
resources that put arrays of every form at the hoisted leaves, wave by wave. Statuses and the
path of every failing pair against the oracle, on both engines, at batch sizes around one wave
and at one full workgroup plus a partial one."""
import numpy as np
import pytest

import hoist_words_data as data
from kyverno_amd import batch
from parity_util import compare

pytestmark = pytest.mark.gpu

N_RULES = data.N_IMAGE + 6


@pytest.fixture(scope="module")
def inputs():
    return data.policies(), data.resources()


@pytest.mark.parametrize("n_res", [1, 63, 64, 65, 320])
@pytest.mark.parametrize("specialize", [True, False])
def test_hoist_words_parity(orc, inputs, monkeypatch, specialize, n_res):
    pols, ress = inputs
    ress = ress[:n_res]
    # the cap on compared failure paths is resources x rules, the size of the status matrix: the
    # pairs that fail on both sides cannot outnumber it, so compare() samples none of them
    max_pairs = n_res * N_RULES
    seen = []
    path = batch.Result.path

    def counted(self, rule, res):
        seen.append((rule, res))
        return path(self, rule, res)

    monkeypatch.setattr(batch.Result, "path", counted)
    mism, r, ost = compare(orc, pols, ress, max_path_checks=max_pairs, specialize=specialize)
    assert ost.shape == (N_RULES, n_res) and max_pairs == ost.size
    # every pair that fails on both sides had its path compared, once
    both = {(int(a), int(b)) for a, b in np.argwhere((r.status == 1) & (ost == 1))}
    assert len(seen) == len(both) and set(seen) == both
    assert n_res < 63 or len(both) > 400  # (more than compare()'s default sample)
    assert not mism, mism[:20]
    if n_res == data.N_RES:
        for rule in range(N_RULES):
            assert (r.status[rule] == 0).any() and (r.status[rule] == 1).any(), rule
    if specialize:
        info = batch.PolicySet(pols, specialize=True).jit_info
        assert info["kernels"] == 1 and info["cols_wide"] >= 1 and info["cols_narrow"] >= 3, info
