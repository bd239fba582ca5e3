"""tests/kvemu.py with every foreach compile flag (KV_COMPILE_FOREACH | _PATTERN | _ENTRIES |
_ANYPATTERN | _PATVARS), next to kvemu_anypattern.py: the generated source of a policy set compiled
with them, built for the host under ASan/UBSan, and a run of it. The emulator fills the rows of the
pattern sets and any sets with variable strings through tools/kvemu/fepat.cpp: the host build of
kv_fe_subst and of the walk's element-rooted dynamic leaf, as kv_foreach_patv_kernel and
kv_foreach_anyv_kernel run them.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess

import numpy as np

import kvemu

FLAGS = dict(foreach=True, foreach_pattern=True, foreach_entries=True, foreach_anypattern=True, foreach_patvars=True)


def build(policies, workdir: str, opt: str = "-O1") -> str:
    from kyverno_amd import batch

    kvemu.build_host()
    os.makedirs(workdir, exist_ok=True)
    src = os.path.join(workdir, "gen.cpp")
    kvemu._with_env({"KVGPU_JIT_DUMP": src, "KVGPU_JIT_SKIP_COMPILE": "1"},
                    lambda: batch.PolicySet(policies, specialize=True, **FLAGS))
    data = open(src, "rb").read()
    host = hashlib.sha1(open(kvemu.HOSTLIB, "rb").read()).hexdigest()
    tag = hashlib.sha1(data + opt.encode() + host.encode() + b"foreach-patvars").hexdigest()[:12]
    exe = os.path.join(workdir, f"kvemu_{tag}")
    if not os.path.exists(exe):
        obj = os.path.join(workdir, f"gen_{tag}.o")
        subprocess.run([kvemu.CLANG, opt, "-g0", "-std=c++17", *kvemu.SAN, "-w", "-include",
                        os.path.join(kvemu.EMU, "shim.h"), "-x", "c++", src, "-c", "-o", obj], check=True)
        subprocess.run([kvemu.HIPCC, *kvemu.SAN, "-rdynamic", obj, kvemu.HOSTLIB, "-o", exe, "-ldl", "-lpthread",
                        "-L/opt/rocm/lib", "-lhiprtc", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"], check=True,
                       stderr=subprocess.DEVNULL)
    with open(os.path.join(workdir, "policies.json"), "w") as f:
        json.dump(policies, f)
    return exe


def run(exe: str, resources: bytes, workdir: str, timeout: int = 1800) -> np.ndarray:
    """Statuses [rules][res] of an emulator run with the five foreach flags."""
    from kyverno_amd import batch

    rpath = os.path.join(workdir, "resources.ndjson")
    with open(rpath, "wb") as f:
        f.write(resources)
    out = os.path.join(workdir, "out")
    e = dict(os.environ)
    e["KVEMU_COMPILE_FLAGS"] = str(batch.COMPILE_FOREACH | batch.COMPILE_FOREACH_PATTERN | batch.COMPILE_FOREACH_ENTRIES
                                   | batch.COMPILE_FOREACH_ANYPATTERN | batch.COMPILE_FOREACH_PATVARS)
    e["KVEMU_NO_ERR"] = "1"
    e["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0"
    e["UBSAN_OPTIONS"] = "print_stacktrace=1"
    p = subprocess.run([exe, os.path.join(workdir, "policies.json"), rpath, "-", out], env=e, capture_output=True,
                       timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"kvemu failed ({p.returncode}):\n{p.stderr.decode(errors='replace')[-6000:]}")
    nr, nres, _wide = map(int, open(out + ".meta").read().split())
    return np.fromfile(out + ".status", dtype=np.uint8).reshape(nr, nres)
