"""Host-side reading of a fetched result (kyverno_amd/csrc/kvresult.cpp) without a device, under
ASan/UBSan: tools/kvemu/result_check builds kv_results by hand from an expected status matrix in
every form a fetch produces (dense store order, the packed transfer form, the caller's order; one
part and three shard parts) and prints what the status matrices and the per-pair message accessors
give. The inputs are the crafted precondition, deny and foreach sets of the GPU tests with their
expected side as the matrix; the assertions on the messages are those of tests/test_gpu_*.py.

Sizes: 1, 255 / 256 / 257 (the edges of a 256-status segment of the transfer form and of the
32-status step of its unpack) and 513 (the size the GPU tests cut into parts)."""
import json
import os
import subprocess

import numpy as np
import pytest

import deny_data as dd
import foreach_data as fd
import kvemu
import precond_data as pd
from kyverno_amd import batch, cli

SIZES = [1, 255, 256, 257, 513]
SETS = {"precond": (pd, 0), "deny": (dd, batch.COMPILE_DENY), "foreach": (fd, batch.COMPILE_FOREACH)}
EXE = os.path.join(kvemu.ROOT, "build", "kvemu", "result_check")
FORMS = ["dense1", "packed1", "packed_sc1", "dense3", "packed3", "packed_sc3"]  # (packed_sc: status_caller() first)
TEXTS = ("subst_error", "precond_message", "deny_message", "foreach_message")
_cache = {}


def _checked(orc, tmp_path_factory, kind, n):
    """(policy, resources, expected side, result_check's output) of one set at one size, run once."""
    if (kind, n) in _cache:
        return _cache[(kind, n)]
    kvemu.build_host()
    mod, flags = SETS[kind]
    pol, ress = mod.crafted_policy(), mod.crafted_resources(n)
    exp = mod.Expected(orc, pol, ress)
    d = tmp_path_factory.mktemp(f"result_{kind}_{n}")
    (d / "policies.json").write_text(json.dumps([pol]))
    (d / "resources.json").write_text(json.dumps(ress))
    exp.status.astype(np.uint8).tofile(str(d / "status.u8"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([EXE, str(d / "policies.json"), str(d / "resources.json"), str(flags), str(d / "status.u8")],
                       env=env, capture_output=True, timeout=120)
    # (a sanitizer report ends the program with a non-zero status; an unpermuted store does too)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode(errors="replace")[-4000:]
    out = json.loads(p.stdout)
    for f in out["forms"]:
        for name in TEXTS + ("foreach_element",):
            vals = {(a, k): v for a, k, v in f[name]}
            assert len(vals) == len(f[name])
            # (no accessor fails on a pair of a result with statuses)
            assert not [x for x in vals.items() if not isinstance(x[1], str if name in TEXTS else int) or x[1] == ""][:5]
            f[name] = vals
    _cache[(kind, n)] = (pol, ress, exp, out)
    return _cache[(kind, n)]


CASES = pytest.mark.parametrize("n", SIZES)


def _forms(out, n):
    """Every form is there: the caller's order too once the store is permuted (n > 1)."""
    want = FORMS + (["caller1"] if n > 1 else [])
    assert sorted(f["name"] for f in out["forms"]) == sorted(want)
    assert (len(out["order"]) == n) == (n > 1)
    return out["forms"]


@pytest.mark.parametrize("kind", list(SETS))
@CASES
def test_status_matrices(orc, tmp_path_factory, kind, n):
    """status_caller() is the input; st_store() is the input in the order the form keeps (the
    batch's store order, mapped back through Batch::order, or the caller's)."""
    pol, ress, exp, out = _checked(orc, tmp_path_factory, kind, n)
    want = exp.status.astype(np.uint8)
    assert (out["n_rules"], out["n_res"]) == want.shape
    order = np.asarray(out["order"], dtype=np.int64) if out["order"] else np.arange(n)
    assert sorted(order.tolist()) == list(range(n))
    for f in _forms(out, n):
        assert f["parts"] == (3 if f["name"].endswith("3") else 1)
        assert np.array_equal(np.asarray(f["status_caller"], dtype=np.uint8).reshape(want.shape), want), f["name"]
        st = np.asarray(f["st_store"], dtype=np.uint8).reshape(want.shape)
        assert f["order"] == ("caller" if f["name"] == "caller1" else "store")
        back = st if f["order"] == "caller" else st[:, np.argsort(order)]  # st[:, s] is caller order[s]
        assert np.array_equal(back, want), f["name"]


@CASES
def test_precondition_messages(orc, tmp_path_factory, n):
    """tests/test_gpu_preconditions.py: "preconditions not met" exactly on the gated pairs."""
    pol, ress, exp, out = _checked(orc, tmp_path_factory, "precond", n)
    pairs = np.argwhere((exp.status == cli.FAIL) | (exp.status == cli.SKIP) | (exp.status == cli.ERROR))
    assert n == 1 or exp.gated.any()
    for f in _forms(out, n):
        pm = f["precond_message"]
        for ri, k in pairs:
            assert (pm.get((int(ri), int(k))) == pd.NOT_MET) == bool(exp.gated[ri, k]), (f["name"], ri, k)
        for ri, k in np.argwhere(exp.status == cli.PASS)[:40]:  # other statuses have no precondition message
            assert pm.get((int(ri), int(k))) is None


@CASES
def test_deny_messages(orc, tmp_path_factory, n):
    """tests/test_gpu_deny.py: a deny message exactly on the ERROR pairs of a deny rule, one of the
    model's; the gate's message exactly on the gated pairs; none for other causes."""
    pol, ress, exp, out = _checked(orc, tmp_path_factory, "deny", n)
    names = [x["name"] for x in pol["spec"]["rules"]]
    pp = names.index("plain-pattern")
    for f in _forms(out, n):
        dm, pm = f["deny_message"], f["precond_message"]
        for (ri, k), msgs in exp.messages.items():
            st = int(exp.status[ri, k])
            assert (dm.get((ri, k)) is not None) == (st == cli.ERROR), (f["name"], names[ri], k)
            if st == cli.ERROR:
                assert dm[(ri, k)] in msgs, (f["name"], names[ri], k)
            assert (pm.get((ri, k)) == dd.NOT_MET) == bool(exp.gated[ri, k]), (f["name"], names[ri], k)
        for k in range(min(n, 40)):
            assert dm.get((pp, k)) is None
        for ri, k in np.argwhere((exp.status == cli.CPU) | (exp.status == cli.NOMATCH))[:40]:
            assert dm.get((int(ri), int(k))) is None


@CASES
def test_foreach_messages_and_elements(orc, tmp_path_factory, n):
    """tests/test_gpu_foreach.py: the foreach message by status, the deciding element of every
    pair, no deny message on a foreach rule."""
    pol, ress, exp, out = _checked(orc, tmp_path_factory, "foreach", n)
    names = [x["name"] for x in pol["spec"]["rules"]]
    for f in _forms(out, n):
        dm, pm, fm, fe = f["deny_message"], f["precond_message"], f["foreach_message"], f["foreach_element"]
        for (ri, k), msgs in exp.messages.items():
            assert dm.get((ri, k)) is None, (f["name"], names[ri], k)
            assert (pm.get((ri, k)) == fd.NOT_MET) == bool(exp.gated[ri, k]), (f["name"], names[ri], k)
            st, got = int(exp.status[ri, k]), fm.get((ri, k))
            if st == cli.ERROR:
                assert got is not None and got in msgs, (f["name"], names[ri], k)
            elif st == cli.SKIP:
                assert got == (None if exp.gated[ri, k] else "rule skipped"), (f["name"], names[ri], k)
            else:
                assert got is None, (f["name"], names[ri], k)
        for ri in range(len(names)):
            for k in range(n):
                assert fe.get((ri, k)) == exp.elem.get((ri, k)), (f["name"], names[ri], k)
