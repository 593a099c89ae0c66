"""The host batch pipeline's planning code (juicefs_amd/csrc/batch_plan.h:
chunk planner, staging layout, copy pieces, LZ4 small-batch geometry) on a
CPU.  tests/batch_plan_check.cc is a stand-alone program built against the
header with AddressSanitizer + UBSan (a plain build where the toolchain has no
sanitizers) and run here; it checks fixed chunk tables and invariants over
seeded random block lists."""
import os
import subprocess
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_plan_tables_and_invariants(tmp_path):
    src = os.path.join(ROOT, "tests", "batch_plan_check.cc")
    exe = str(tmp_path / "batch_plan_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", src, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:  # no sanitizer runtime: the checks still run, and the run says so
        warnings.warn("batch_plan_check built WITHOUT ASan/UBSan: " + r.stderr[-300:])
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    print("batch_plan_check build:", "ASan+UBSan" if sanitized else "plain")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "batch plan check OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
