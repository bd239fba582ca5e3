"""The end-of-kernel flush of the specialized rule kernels (kvdevfn.h kv_end_flush) against the
oracle: status matrix, per-rule counts and per-namespace counts, over the sizes at which the
flush takes another path.

Rules per kernel: 1; 16 (one iteration of the copy and sum loops exactly); 17 (one iteration and
a one-row tail); 100; 128 (KV_KROWS: 8 iterations, every slot of the rule-id table in use). The
sets are prefixes of the C2 rules, one rule per policy (so the oracle's per-pair call that
compare() makes for every failing path evaluates one rule), plus renamed copies with changed
constants up to 128.

Resources: 1; 64; 256 (one full workgroup, 16 B stores); 272 (the 16 B path, then a partial
workgroup on the byte path); 273 (rows not 16 B aligned: every workgroup on the byte path); 767.
Namespaces are laid out so that the first 64-resource wave holds three of them and the
workgroups span two (the store is ordered by namespace): per-scope counts take the other-scope
path as well as the workgroup's own.
"""
import copy
import json

import numpy as np
import pytest

from kyverno_amd import batch, workloads
from parity_util import compare, oracle_status

pytestmark = pytest.mark.gpu

N_MAX = 767
RULES = [1, 16, 17, 100, 128]
RESOURCES = [1, 64, 256, 272, 273, N_MAX]
# namespace of the resource at position i of the namespace-ordered store: [first position, name)
NS_LAYOUT = [(0, "ns-fa"), (20, "ns-fb"), (40, "ns-fc"), (70, "ns-fd"), (400, "ns-fe")]


def _extra_rules():
    """28 renamed copies of C2 rules with other constants (100 + 28 = KV_KROWS)."""
    base = {r["name"]: r for r in workloads.c2_policies()[0]["spec"]["rules"]}
    out = []
    globs = ["*:v2.*", "!*:v1.*", "quay.io/*", "!gcr.io/*", "*app*", "!*nginx*:latest", "*:v?.?.*", "docker.io/* | gcr.io/*",
             "!*@sha256:a*", "*-2?:*", "*/*", "!*:v3.*", "*redis*", "!quay.io/*:latest", "*.local:5000/*", "*:v1.2?.*",
             "!docker.io/nginx*", "*b*", "!*:v9.*", "??*"]
    for i, g in enumerate(globs):
        r = copy.deepcopy(base[f"image-{i:02d}"])
        r["name"] = f"image-x{i:02d}"
        r["validate"]["pattern"]["spec"]["containers"][0]["image"] = g
        r["validate"]["message"] = f"image must match {g}"
        out.append(r)
    quant = [("limits", "memory", "<=3Gi"), ("limits", "memory", ">=64Mi"), ("requests", "memory", "<=2Gi"),
             ("requests", "cpu", "<=2"), ("requests", "cpu", "50m-1"), ("limits", "cpu", ">=100m"),
             ("limits", "cpu", "!2"), ("requests", "memory", "128Mi-2Gi")]
    for i, (grp, res, pat) in enumerate(quant):
        r = copy.deepcopy(base["quantity-00"])
        r["name"] = f"quantity-x{i:02d}"
        r["validate"]["pattern"] = {"spec": {"containers": [{"=(resources)": {f"=({grp})": {f"=({res})": pat}}}]}}
        out.append(r)
    assert len(out) == 28
    return out


def _policies(rules):
    return [workloads._policy(f"flush-{i:03d}", [r]) for i, r in enumerate(rules)]


def _resources(n, layout):
    ress = [json.loads(line) for line in batch.synth(workloads.SEED + 11, n).decode().strip().split("\n")]
    for i, r in enumerate(ress):
        r["metadata"]["namespace"] = [ns for first, ns in layout if first <= i][-1]
    return ress


@pytest.fixture(scope="module")
def inputs(orc):
    """Per rule count: the policies, their compiled set and the oracle's statuses of the N_MAX
    resources (a case with fewer resources takes the first of them: the matrix's leading columns)."""
    rules = workloads.c2_policies()[0]["spec"]["rules"] + _extra_rules()
    ress = _resources(N_MAX, NS_LAYOUT)
    sets = {}

    def get(n_rules):
        if n_rules not in sets:
            pols = _policies(rules[:n_rules])
            ps = batch.PolicySet(pols, specialize=True)
            assert ps.jit_info["kernels"] == 1, ps.jit_info
            ost = oracle_status(orc, pols, ress)
            assert ost.shape == (n_rules, N_MAX)
            ost.flags.writeable = False
            sets[n_rules] = (pols, ps, ost)
        return sets[n_rules]

    return ress, get


def _histogram(ost):
    want = np.zeros((ost.shape[0], 8), np.int64)
    np.add.at(want, (np.arange(ost.shape[0])[:, None], ost), 1)
    return want


@pytest.mark.parametrize("n_res", RESOURCES)
@pytest.mark.parametrize("n_rules", RULES)
def test_full_status_and_paths(orc, inputs, n_rules, n_res):
    ress, get = inputs
    pols, ps, ost = get(n_rules)
    # (the cap on compared failing paths is the matrix size: compare() samples none)
    mism, r, o = compare(orc, pols, ress[:n_res], max_path_checks=n_rules * n_res, specialize=True)
    assert not mism, mism[:20]
    assert np.array_equal(o, ost[:, :n_res])
    assert np.array_equal(r.status, ost[:, :n_res])
    assert np.array_equal(r.counts, _histogram(ost[:, :n_res]))


@pytest.mark.parametrize("n_res", RESOURCES)
@pytest.mark.parametrize("n_rules", RULES)
def test_counts(inputs, n_rules, n_res):
    ress, get = inputs
    pols, ps, ost = get(n_rules)
    b = batch.Batch(ps, ress[:n_res])
    sess = batch.Session(ps, b, mode=batch.MODE_COUNTS)
    sess.run(1)
    assert np.array_equal(sess.counts(), _histogram(ost[:, :n_res]))


@pytest.mark.parametrize("n_res", RESOURCES)
@pytest.mark.parametrize("n_rules", RULES)
def test_scope_counts(inputs, n_rules, n_res):
    ress, get = inputs
    pols, ps, ost = get(n_rules)
    b = batch.Batch(ps, ress[:n_res])
    nss = b.namespaces
    idx = {n: i for i, n in enumerate(nss)}
    assert len(nss) == sum(1 for first, _ in NS_LAYOUT if first < n_res)
    want = np.zeros((len(nss), n_rules, 8), np.int64)
    for j, r in enumerate(ress[:n_res]):
        np.add.at(want[idx[r["metadata"]["namespace"]]], (np.arange(n_rules), ost[:, j]), 1)
    sess = batch.Session(ps, b, mode=batch.MODE_SCOPES | batch.MODE_COUNTS)
    sess.run(1)
    assert np.array_equal(sess.scope_counts(len(nss)), want)


def test_unwritten_segments(orc):
    """A rule that matches one namespace only: the 256-status segments of the workgroups that hold
    none of its resources are all NOMATCH and are not written (DevOut::sflag 0; the fetch fills
    them). 3 x 304 resources (a multiple of 16, so the full workgroups take the 16 B path):
    workgroup 0 holds ns-ga only, workgroup 1 ns-ga and ns-gb, workgroup 2 ns-gb and ns-gc,
    workgroup 3 is partial."""
    n = 3 * 304
    ress = _resources(n, [(0, "ns-ga"), (304, "ns-gb"), (608, "ns-gc")])
    rules = copy.deepcopy(workloads.c2_policies()[0]["spec"]["rules"][:16])
    only = copy.deepcopy(rules[0])
    only["name"] = "only-gc"
    only["match"] = {"resources": {"kinds": ["Pod"], "namespaces": ["ns-gc"]}}
    rules.append(only)
    pols = _policies(rules)
    ps = batch.PolicySet(pols, specialize=True)
    assert ps.jit_info["kernels"] == 1, ps.jit_info
    b = batch.Batch(ps, ress)
    ost = oracle_status(orc, pols, ress)
    assert (ost[16, :608] == 5).all() and (ost[16, 608:] != 5).all()
    sess = batch.Session(ps, b, mode=batch.MODE_STATUS | batch.MODE_ERRORS)
    sess.run(1)
    assert sess.status_bytes() < len(rules) * n
    # (the rule's segments of workgroups 0 and 1 at the least)
    assert sess.status_bytes() <= len(rules) * n - 512
    r = sess.fetch()
    assert np.array_equal(r.status, ost)
    assert np.array_equal(r.counts, _histogram(ost))
