"""The build half of the specialized kernels (kyverno_amd/csrc/kvjitbuild.cpp) without a device and
without a compile, under ASan/UBSan: tools/kvemu/jitbuild_check checks the register verdict over
priv {0, 16} x calls x waves {0, 1, 6, 8} x vgprs {64, 72, 88, 512} against the rules of the spill
plan, the variants and the block probes written out; every rung of the spill plan's ladder on
hand-built images with injected verdicts; and the plan file's round trip, with malformed files
rejected. On the generator's side (kvjitgen.cpp) it generates a small hand-written policy set, two
rules per kernel, and checks that every kernel program ends with its own kernel and defines every
g_ / q_ / r_ helper it uses before the use."""
import json
import os
import subprocess

import kvemu

EXE = os.path.join(kvemu.ROOT, "build", "kvemu", "jitbuild_check")


def test_jitbuild_check(tmp_path):
    kvemu.build_host()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([EXE, str(tmp_path)], env=env, capture_output=True, timeout=120)
    # (a sanitizer report ends the program with a non-zero status; a failed check prints its line)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode(errors="replace")[-4000:]
    out = json.loads(p.stdout)
    assert out["failed"] == 0 and out["checks"] > 64 * 5
    assert sorted(os.listdir(tmp_path))[-1] == "plan-roundtrip.txt"  # (the plan file is in the given cache)
