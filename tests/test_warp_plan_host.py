"""CPU: csrc/warp_plan.h (what svt_hip_warp_fit_frame and svt_hip_warp_pred_frame decide on the host before they enqueue) as a stand-alone
program, built plain and under AddressSanitizer + UBSan (host code with its own main)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cidana-svt-av1_amd")


@pytest.mark.parametrize("san_flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_warp_plan(tmp_path, san_flags):
    """every clause of warp_fit_check and warp_pred_check refuses its one changed field; the tiling of every plane block shape; a mixed
    list's workgroup counts and group tables against hand-computed values; lists longer than one launch's table; the filter tables"""
    exe = str(tmp_path / "warp_plan_host")
    pr = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror"] + san_flags +
                        [os.path.join(ROOT, "tests", "c", "warp_plan_host.cpp"), os.path.join(PKG, "csrc", "host_err.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip() == "ok"
