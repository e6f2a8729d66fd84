"""CPU: csrc/me_plan.h and csrc/pixel_plan.h (what the motion-estimation and pixel calls settle on the host before they enqueue: every
refusal in the order a caller observes it, the kernel of a full-pel search, the grids and LDS windows, the frame call's plan with the
host-side rules of MotionEstimateLcu) as a stand-alone program, built plain and under AddressSanitizer + UBSan (host code with its own
main, run directly)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cidana-svt-av1_amd")


@pytest.mark.parametrize("san_flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_me_plan(tmp_path, san_flags):
    """for every entry point of the family a valid argument set is accepted and, clause by clause, the same set with one field changed is
    refused with SVT_HIP_ERR_INVALID and the text the entry point gave before the plan existed, the four cases where two clauses fail at
    once included; the frame plan's scratch equals the header's formula, every enabled HME level's regions are present and fit the one
    window the prologue stages, within the LDS bounds; the full-pel routing takes the 16-points-per-lane kernel only inside 60 KiB, the
    four-points one only on widths that are multiples of 8 inside 58 KiB, the general kernel otherwise and under the knob; hme_list,
    second_best, zz_check and the bi-prediction switches equal a table written from EbMotionEstimation.c over slice type x temporal layer x
    same-POC x levels x cu8x8_mode x PU count x method; the residual's lanes tile the row, its grid covers the batch and pow2 is exact;
    the SAD grid covers the batch at 16 blocks per workgroup and x4d refuses above 0x3fffffff; every recorded launch of the GPU tests and
    the tools equals what the entry points computed before the plan existed, and every kernel of the family appears among them"""
    exe = str(tmp_path / "me_plan_host")
    pr = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror"] + san_flags +
                        [os.path.join(ROOT, "tests", "c", "me_plan_host.cpp"), os.path.join(PKG, "csrc", "host_err.cpp"),
                         os.path.join(PKG, "csrc", "host_tables.cpp"), "-o", exe], capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip() == "ok"
