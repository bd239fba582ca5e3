"""Narrow path-column cells on the device: the narrow_cols_data policies and resources (every
kind of value at a root leaf and at an element leaf, arrays at leaf positions, padded element
rows, a map column whose node index is read) and the C2 policy set on synthetic Pods, statuses
and failure paths against the oracle."""
import json

import numpy as np
import pytest

import narrow_cols_data as data
from parity_util import compare

pytestmark = pytest.mark.gpu

MAX_PAIRS = data.N_RES * 4  # 320 resources x 4 rules: every failing path is compared, none sampled


@pytest.mark.parametrize("specialize", [True, False])
def test_narrow_cols_parity(orc, specialize):
    pols, ress = data.policies(), data.resources()
    mism, r, ost = compare(orc, pols, ress, max_path_checks=MAX_PAIRS, specialize=specialize)
    assert int((ost == 1).sum()) <= MAX_PAIRS
    assert not mism, mism[:20]
    for rule in range(ost.shape[0]):
        assert (r.status[rule] == 0).any() and (r.status[rule] == 1).any(), rule
    if specialize:
        from kyverno_amd import batch

        info = batch.PolicySet(pols, specialize=True).jit_info
        assert info["cols_wide"] >= 1 and info["cols_narrow"] >= 1, info


def test_c2_narrow_cols_parity(orc):
    from kyverno_amd import batch, workloads

    pols = workloads.c2_policies()
    ress = [json.loads(x) for x in batch.synth(workloads.SEED, 300).decode().strip().split("\n")]
    # (30 000 pairs: the failure paths of a fixed sample of 400 failing pairs keep the test short)
    mism, r, ost = compare(orc, pols, ress, specialize=True)
    assert not mism, mism[:20]
    assert (ost == 0).any() and (ost == 1).any()
    assert np.array_equal(r.status, ost)
