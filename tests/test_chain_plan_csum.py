"""The read calls' disk-cache checksum planning (juicefs_amd/csrc/chain_plan.h:
chain_csum_pieces, the "reads' checksums" flag of ChainLayout) on a CPU.
tests/chain_plan_csum_check.cc is a stand-alone program built against the
header with AddressSanitizer + UBSan (a plain build where the toolchain has no
sanitizers) and run here; it checks the piece prefix and checksum offsets
around the 32 KiB piece for every wanted / not-wanted mask, that the layout of
a call without checksums is field by field what it was before the flag, and
that with the flag on no two areas overlap and each lies inside its copy."""
import os
import subprocess
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_plan_csum_pieces_and_layout(tmp_path):
    src = os.path.join(ROOT, "tests", "chain_plan_csum_check.cc")
    exe = str(tmp_path / "chain_plan_csum_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", src, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:  # no sanitizer runtime: the checks still run, and the run says so
        warnings.warn("chain_plan_csum_check built WITHOUT ASan/UBSan: " + r.stderr[-300:])
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    print("chain_plan_csum_check build:", "ASan+UBSan" if sanitized else "plain")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "chain plan csum check OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
