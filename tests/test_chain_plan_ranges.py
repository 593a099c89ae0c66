"""The read calls' sparse-mode planning (juicefs_amd/csrc/chain_plan.h:
chain_ranges, the lists' area of ChainLayout) on a CPU.
tests/chain_plan_ranges_check.cc is a stand-alone program built against the
header with AddressSanitizer + UBSan and run here; it checks that the ranges of
the segments that reference a source are clamped to its capacity, sorted and
merged where they overlap or touch, that holes and unreferenced sources add
nothing, the running sums, and that the layout of a call without lists is what
it was while one with lists keeps its two new areas inside the H2D copy."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_plan_ranges_and_layout(tmp_path):
    src = os.path.join(ROOT, "tests", "chain_plan_ranges_check.cc")
    exe = str(tmp_path / "chain_plan_ranges_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "chain plan ranges check OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
