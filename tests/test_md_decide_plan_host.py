"""CPU: the decide of mode decision in csrc/md_plan.h (what svt_hip_md_decide_frame and svt_hip_md_search_frame settle on the host before
they enqueue) as a stand-alone program, built plain and under AddressSanitizer + UBSan (host code with its own main, run directly)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cidana-svt-av1_amd")


@pytest.mark.parametrize("san_flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_md_decide_plan(tmp_path, san_flags):
    """every clause of md_decide_check refuses its one changed field (bsize 13 .. 15, n, the candidate counts, full_loop_escape, NULL and
    misaligned members, Cb without Cr, a gather without its input or equal to it, the 31-bit bound) and accepts the neighbour of each
    bound; the wave-unit of every block size and slot count fits the kernel's tile and gather budget; the scratch size, the carving
    (aligned, in order, no overlap, inside a scratch of exactly the reported size) and the stage groups of the composed search against
    hand-computed values"""
    exe = str(tmp_path / "md_decide_plan_host")
    pr = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror"] + san_flags +
                        [os.path.join(ROOT, "tests", "c", "md_decide_plan_host.cpp"), os.path.join(PKG, "csrc", "host_tables.cpp"),
                         os.path.join(PKG, "csrc", "host_err.cpp"), "-o", exe], capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip() == "ok"
