"""Per-rule and nested array loops read from path columns, on the device: the col_loops_data
policies (a nested loop, an existence anchor over a root array, both forms in rules of one form,
a rule with a fused and a nested loop over one parent) on both engines against the oracle:
statuses and the path of every failing pair, at 64 + 7 resources (a full wave and a partial one)
and at 256 + 64 + 5 (a full workgroup, a full wave and a partial one, so the rows of the nested
family are offset across wave groups)."""
import numpy as np
import pytest

import col_loops_data as data
from kyverno_amd import batch
from parity_util import compare

pytestmark = pytest.mark.gpu

N_RULES = len(data.RULES)


@pytest.fixture(scope="module")
def inputs():
    return data.policies(), data.resources()


@pytest.mark.parametrize("n_res", [data.N_SMALL, data.N_RES])
@pytest.mark.parametrize("specialize", [True, False])
def test_col_loops_parity(orc, inputs, monkeypatch, specialize, n_res):
    pols, ress = inputs
    ress = ress[:n_res]
    # the cap on compared failure paths is the size of the status matrix, so compare() samples none
    max_pairs = n_res * N_RULES
    seen = []
    path = batch.Result.path

    def counted(self, rule, res):
        seen.append((rule, res))
        return path(self, rule, res)

    monkeypatch.setattr(batch.Result, "path", counted)
    mism, r, ost = compare(orc, pols, ress, max_path_checks=max_pairs, specialize=specialize)
    assert ost.shape == (N_RULES, n_res)
    both = {(int(a), int(b)) for a, b in np.argwhere((r.status == 1) & (ost == 1))}
    assert len(seen) == len(both) and set(seen) == both and len(both) > 300
    assert not mism, mism[:20]
    for rule in range(N_RULES):
        assert (r.status[rule] == 0).any() and (r.status[rule] == 1).any(), rule
    if specialize:
        info = batch.PolicySet(pols, specialize=True).jit_info
        assert info["kernels"] == 1, info
