#!/usr/bin/env python3
"""Static ISA report of the specialized kernels of a workload (no GPU needed).

Compiles the workload's policy set (through the code-object cache, KVGPU_JIT_CACHE), dumps
the final code objects (KVGPU_JIT_DUMP_CO) and prints per rule kernel: VGPRs, SGPRs, SGPR
spills (into VGPR lanes), private segment, code bytes, and the static instruction mix
(scalar ALU, exec-mask control flow, vector ALU, memory). The generated rule kernels run
nearly all of their code in every wave (some lane of 64 takes almost every branch), so the
static mix tracks the dynamic issue load (SQ_INSTS_SALU / SQ_INSTS_VALU).

Memory waits: per kernel the static counts of vector-memory loads (`ld`) and of `s_waitcnt`
with a vmcnt field (`wait`), and one line per fused-loop body (an outermost loop of at least
LOOP_MIN instructions): its loads, waits and rounds, and those of its head. A round is a wait
with a load issued since the wait before it: the waits of one round drain loads that were in
flight together, so rounds, not waits, count the memory round trips a wave sits through. The
head is the code from the body's first load up to the next instruction that touches the exec
mask. A hoist region (kvjitgen.cpp HoistTable::flush) has no branch before its first rule
body, so the head holds the region's cell loads and word gathers: one round for the cells in
the head, and one for the words where the first rule reads one.

Single-load waits (`one`): the waits before which exactly one load was issued since the wait
before them. A chain of them is a walk of the node rows, each load waiting for the one before
it (a cursor's type, its map's slot, the child); the lookups of a hoist region share their
waits instead. Per kernel (column `one`) and per loop.

End flush (`flush`): one line per kernel for the code from the entry barrier of kv_end_flush
(kvdevfn.h) to s_endpgm: its instructions, vector-memory loads, `s_waitcnt`s with a vmcnt field,
stores and atomics. Stores and atomics count in vmcnt with the loads, so a load's wait in this
region also drains every store and atomic before it; the flush reads its rule ids ahead of the
entry barrier and should show no load and no wait here. The entry barrier is found from the
end, since the prefill has a barrier of its own near the kernel start: the flush has three
barriers where the kernel copies statuses (entry, after the copy, after the count phase), so
the entry barrier is the third from the end; a variant that writes no status matrix (.m8) has
no copy loop and no middle barrier, and the kernel then has three barriers in all: there the
entry barrier is the second from the end. (At run time the byte path of a partial workgroup
skips the middle barrier too; statically it is there.)

    python tools/jit_isa.py [c2|c3|c4|c5] [--env K=V ...]
"""
import collections
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

args = sys.argv[1:]
wl = args[0] if args and not args[0].startswith("--") else "c2"
for a in args:
    if "=" in a and not a.startswith("--"):
        k, v = a.split("=", 1)
        os.environ[k] = v
os.environ.setdefault("KVGPU_JIT_CACHE", os.path.join(ROOT, "kyverno_amd", "jitcache"))
d = tempfile.mkdtemp()
os.environ["KVGPU_JIT_DUMP_CO"] = os.path.join(d, "k")
from kyverno_amd import batch, workloads  # noqa: E402

pols = workloads.c3_policies(1000) if wl == "c3" else getattr(workloads, wl + "_policies")()
ps = batch.PolicySet(pols, specialize=True)
CTRL = {"s_and_saveexec_b64", "s_or_saveexec_b64", "s_andn2_saveexec_b64", "s_cbranch_execz", "s_cbranch_execnz",
        "s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz", "s_branch"}
LOOP_MIN = 300
INST = re.compile(r"^\s+([a-z][a-z0-9_]+)([^/\n]*)//\s*([0-9A-F]+):[^<\n]*(?:<[^+>]+\+0x([0-9a-f]+)>)?", re.M)


def is_load(o):
    return o.startswith(("global_load", "flat_load", "buffer_load", "scratch_load"))


def is_wait(o, rest):
    return o == "s_waitcnt" and "vmcnt" in rest


def loop_report(dis):
    """[(instructions, (loads, waits, rounds, single-load waits), the same of the head)] of the outermost
    large loops"""

    def lwr(xs):
        ld = wt = rd = one = 0
        fresh = 0  # loads issued since the last wait
        for _, o, rest, _ in xs:
            if is_load(o):
                ld, fresh = ld + 1, fresh + 1
            elif is_wait(o, rest):
                wt, rd, one, fresh = wt + 1, rd + (fresh > 0), one + (fresh == 1), 0
        return ld, wt, rd, one

    ins = [(int(a, 16), o, rest, int(t, 16) if t else None) for o, rest, a, t in INST.findall(dis)]
    if not ins:
        return []
    base = ins[0][0]
    at = {a: i for i, (a, _, _, _) in enumerate(ins)}
    span = {}  # loop header -> last backward branch to it
    for i, (a, o, _, t) in enumerate(ins):
        if t is not None and o.startswith(("s_cbranch", "s_branch")) and base + t <= a and base + t in at:
            h = at[base + t]
            span[h] = max(span.get(h, i), i)
    loops = sorted((h, e) for h, e in span.items() if e - h >= LOOP_MIN)
    out, end = [], -1
    for h, e in loops:
        if h <= end:  # nested in the previous outermost loop
            continue
        end = e
        body = ins[h:e + 1]
        head = []
        for x in body:
            if head and "exec" in x[1] + x[2]:
                break
            if head or is_load(x[1]):
                head.append(x)
        out.append((len(body), lwr(body), lwr(head)))
    return out


def flush_report(dis):
    """(instructions, loads, vmcnt waits, stores, atomics) from the end flush's entry barrier to s_endpgm;
    None if the kernel has no such region"""
    ins = INST.findall(dis)
    ends = [i for i, x in enumerate(ins) if x[0] == "s_endpgm"]
    if not ends:
        return None
    bars = [i for i, x in enumerate(ins[:ends[0]]) if x[0] == "s_barrier"]
    if len(bars) < 3:
        return None
    reg = ins[bars[-3] if len(bars) >= 4 else bars[-2]:ends[0] + 1]
    return (len(reg), sum(is_load(o) for o, *_ in reg), sum(is_wait(o, rest) for o, rest, *_ in reg),
            sum(o.startswith(("global_store", "flat_store", "buffer_store")) for o, *_ in reg),
            sum(o.startswith(("global_atomic", "flat_atomic", "buffer_atomic")) for o, *_ in reg))


tot = collections.Counter()
print(f"{'kernel':24s} {'vgpr':>4s} {'sgpr':>4s} {'spill':>5s} {'priv':>4s} {'KB':>6s} {'salu':>6s} {'exec':>6s} "
      f"{'valu':>6s} {'lane':>5s} {'vmem':>5s} {'lds':>5s} {'ld':>5s} {'wait':>5s} {'one':>5s}")
for f in sorted(glob.glob(os.path.join(d, "k.*.co"))):
    label = f.split("k.", 1)[1][:-3]
    name = label.split(".m")[0]  # (output-mode variants: <name>.m<full>)
    if not name.startswith("kvj_r"):
        continue
    notes = subprocess.run([READELF, "--notes", f], capture_output=True, text=True).stdout

    def meta(k):
        m = re.search(r"\." + k + r":\s+(\d+)", notes)
        return int(m.group(1)) if m else -1

    dis = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", f], capture_output=True, text=True).stdout
    ops = re.findall(r"^\s+([sv]_[a-z0-9_]+|global_[a-z0-9_]+|ds_[a-z0-9_]+|buffer_[a-z0-9_]+|flat_[a-z0-9_]+)([^/\n]*)",
                     dis, re.M)
    c = collections.Counter()
    fresh = 0  # loads issued since the last wait
    for o, rest in ops:
        c["ld"] += is_load(o)
        c["wait"] += is_wait(o, rest)
        if is_load(o):
            fresh += 1
        elif is_wait(o, rest):
            c["one"] += fresh == 1
            fresh = 0
        if o in CTRL or (o.startswith("s_") and "exec" in o + rest):
            c["exec"] += 1
        elif o.startswith("s_"):
            c["salu"] += 1
        elif o in ("v_readlane_b32", "v_writelane_b32"):
            c["lane"] += 1
        elif o.startswith("v_"):
            c["valu"] += 1
        elif o.startswith("ds_"):
            c["lds"] += 1
        else:
            c["vmem"] += 1
    size = os.path.getsize(f)
    tot.update(c)
    print(f"{label[:24]:24s} {meta('vgpr_count'):4d} {meta('sgpr_count'):4d} {meta('sgpr_spill_count'):5d} "
          f"{meta('private_segment_fixed_size'):4d} {size / 1024:6.0f} {c['salu']:6d} {c['exec']:6d} {c['valu']:6d} "
          f"{c['lane']:5d} {c['vmem']:5d} {c['lds']:5d} {c['ld']:5d} {c['wait']:5d} {c['one']:5d}")
    for k, (n, b, h) in enumerate(loop_report(dis)):
        print(f"  loop {k}: {n:5d} instructions, {b[0]:3d} loads {b[1]:3d} waits {b[2]:3d} rounds {b[3]:3d} single; "
              f"head: {h[0]:2d} loads {h[1]:2d} waits {h[2]:2d} rounds")
    fr = flush_report(dis)
    if fr:
        print(f"  flush: {fr[0]:5d} instructions, {fr[1]:3d} loads {fr[2]:3d} waits {fr[3]:3d} stores {fr[4]:3d} atomics")
print("total", dict(tot))
