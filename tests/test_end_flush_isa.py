"""Static check of the rule kernel's end flush (kvdevfn.h kv_end_flush) in the ISA of C2's FULL
variant: after the flush's entry barrier nothing loads from vector memory, so nothing waits on
vmcnt behind the flush's stores and atomics (on gfx950 stores and atomics count in vmcnt with
the loads: a wait for a load drains them too).

The flush region runs from its entry barrier to s_endpgm. The kernel's first barrier is the
prefill's, so the entry barrier is counted from the end: the FULL variant's flush has three
(entry, after the status copy, after the count phase). The check looks for loads and waits
only."""
import glob
import os
import re
import shutil
import subprocess

import pytest

OBJDUMP = shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"
pytestmark = pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump is absent")

INST = re.compile(r"^\s+([a-z][a-z0-9_]+)([^/\n]*)//\s*([0-9A-F]+):[^<\n]*(?:<[^+>]+\+0x([0-9a-f]+)>)?", re.M)


def test_c2_full_flush_has_no_load_and_no_store_drain(tmp_path, monkeypatch):
    from kyverno_amd import batch, workloads

    monkeypatch.setenv("KVGPU_JIT_DUMP_CO", str(tmp_path / "k"))
    ps = batch.PolicySet(workloads.c2_policies(), specialize=True)
    assert ps.jit_info["kernels"] == 1, ps.jit_info
    cos = glob.glob(str(tmp_path / "k.kvj_r*.m3.co"))
    assert len(cos) == 1, cos
    dis = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", cos[0]], capture_output=True, text=True, check=True).stdout
    ins = [(int(a, 16), o, rest, int(t, 16) if t else None) for o, rest, a, t in INST.findall(dis)]
    base = ins[0][0]
    ends = [i for i, x in enumerate(ins) if x[1] == "s_endpgm"]
    assert len(ends) == 1
    bars = [i for i, x in enumerate(ins[:ends[0]]) if x[1] == "s_barrier"]
    assert len(bars) >= 4, bars  # (the prefill's and the flush's three)
    region = ins[bars[-3]:ends[0] + 1]
    loads = [x for x in region if x[1].startswith(("global_load", "flat_load", "buffer_load", "scratch_load"))]
    assert not loads, [(hex(a), o + rest) for a, o, rest, _ in loads]
    waits = [x for x in region if x[1] == "s_waitcnt" and "vmcnt" in x[2]]
    assert len(waits) <= 1, [(hex(a), o + rest) for a, o, rest, _ in waits]
    # backward branches (loops) as [target, branch] address ranges
    loops = [(base + t, a) for a, o, _, t in ins if t is not None and o.startswith(("s_cbranch", "s_branch")) and base + t <= a]
    for a, o, rest, _ in waits:
        inside = [(hex(lo), hex(hi)) for lo, hi in loops if lo <= a <= hi]
        assert not inside, (hex(a), o + rest, inside)
