#!/usr/bin/env python3
"""The CDEF strength search (svt_hip_cdef_search_frame) and the CDEF apply (svt_hip_cdef_apply_frame) per picture: 1080p 8-bit and
2160p 10-bit, strength windows 0 .. 8 and 0 .. 64, 0 % and 50 % of the 8x8 blocks skipped.  Pictures are low-pass noise with grain
(source) plus coding noise (reconstruction).  Rates are (pixel, strength) pairs per second over the non-skipped pixels of all three
planes.  For context only, where oracle/_ref/libsvtref.so is present: the same 0 .. 64 search of one 1080p picture through the
reference's C functions on one host thread (the fixture generator's loop over cdef_filter_fb / compute_cdef_dist).

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s, 7 windows, median.
Kernel resources (VGPRs, LDS, waves per SIMD) are read from the built library's code objects.
Writes profiles/r06_cdef.json.
    python tools/bench_cdef.py [--out profiles/r06_cdef.json] [--quick] [--no-host]"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import __graft_entry__ as ge  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"


def window(fn, min_s=0.2):
    """seconds per call: calls back to back in a window of >= min_s, HIP events, synchronised around"""
    reps = 1
    while True:
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b) / 1e3
        if t >= min_s:
            return t / reps
        reps = max(reps * 2, int(reps * min_s / max(t, 1e-6) * 1.2) + 1)


def median_of(fn, nwin):
    fn()
    ts = [window(fn) for _ in range(nwin)]
    return statistics.median(ts), ts


def picture(rng, w, h, bd):
    """-> source and reconstruction planes (numpy, uint8 / uint16)"""
    import make_golden_cdef as mg
    cs = bd - 8
    src, rec = [], []
    for pli in range(3):
        s = mg.smooth_picture(rng, h >> (pli > 0), w >> (pli > 0))
        r = (s + rng.integers(-6, 7, s.shape)).clip(0, 255)
        dt = np.uint8 if bd == 8 else np.uint16
        src.append((s << cs).astype(dt))
        rec.append((r << cs).astype(dt))
    return src, rec


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def kernel_resources():
    """the cdef kernels' registers / LDS from the AMDGPU metadata notes of the built library"""
    lib = os.path.join(ROOT, "cidana-svt-av1_amd", "libsvt_hip_dsp.so")
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        return None
    out = []
    with tempfile.TemporaryDirectory() as td:
        shutil.copy(lib, os.path.join(td, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=td, check=True, capture_output=True)
        for f in sorted(os.listdir(td)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=td, check=True, capture_output=True, text=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)
                if "cdef_kernel" not in g("name"):
                    continue
                v = int(g("vgpr_count")) + int(re.match(r"\s*(\d+)", blk).group(1))
                out.append({"kernel": g("name"), "vgprs": v, "sgprs": int(g("sgpr_count")), "lds_bytes": int(g("group_segment_fixed_size")),
                            "scratch_bytes": int(g("private_segment_fixed_size")), "waves_per_simd": min(8, 512 // max(8, -(-v // 8) * 8))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_cdef.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="3 windows, no host reference")
    ap.add_argument("--no-host", action="store_true", help="do not time the reference's C functions on the host")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    nwin = 3 if a.quick else a.windows
    rng = np.random.default_rng(606)
    q = 140
    rows, keep1080 = [], None
    for label, w, h, bd in (("1080p8", 1920, 1080, 8), ("2160p10", 3840, 2160, 10)):
        src, rec = picture(rng, w, h, bd)
        dsrc, drec = tuple(dev(p) for p in src), tuple(dev(p) for p in rec)
        nfb = ((w + 63) // 64) * ((h + 63) // 64)
        for skipped in (0.0, 0.5):
            skip = (rng.random((h // 8, w // 8)) < skipped).astype(np.uint8)
            dskip = dev(skip)
            if label == "1080p8" and skipped == 0.0:
                keep1080 = (src, rec, skip)
            live = int((skip == 0).sum()) * 64 * 3 // 2                     # non-skipped pixels, three planes of 4:2:0
            mse = torch.empty((2, nfb, 64), dtype=torch.int64, device="cuda")
            count = torch.empty(nfb, dtype=torch.int32, device="cuda")
            for g0, g1 in ((0, 8), (0, 64)):
                fn = lambda: dsp.cdef_search_frame(drec, dsrc, dskip, w, h, bd, q, g0, g1, mse=mse, count=count)
                t, raw = median_of(fn, nwin)
                row = {"call": "search", "picture": label, "skipped": skipped, "window": [g0, g1], "ms": round(t * 1e3, 4),
                       "Gpairs_per_s": round(live * (g1 - g0) / t / 1e9, 3), "windows_ms": [round(v * 1e3, 4) for v in raw]}
                print(json.dumps(row), flush=True)
                rows.append(row)
            ys = mse[0].argmin(1).to(torch.int8)
            us = mse[1].argmin(1).to(torch.int8)
            ys[count == 0] = -1
            us[count == 0] = -1
            dst = tuple(torch.empty_like(p) for p in drec)
            t, raw = median_of(lambda: dsp.cdef_apply_frame(drec, dskip, ys, us, w, h, bd, q, dst=dst), nwin)
            row = {"call": "apply", "picture": label, "skipped": skipped, "ms": round(t * 1e3, 4),
                   "GB_per_s": round(2 * (w * h * 3 // 2) * (bd > 8 and 2 or 1) / t / 1e9, 2), "windows_ms": [round(v * 1e3, 4) for v in raw]}
            print(json.dumps(row), flush=True)
            rows.append(row)
        del dsrc, drec
        torch.cuda.empty_cache()
    host = None
    if not (a.quick or a.no_host):
        import make_golden_cdef as mg
        L = mg.ref_lib()
        if L is not None:
            src, rec, skip = keep1080
            t0 = time.perf_counter()
            mg.ref_search(L, rec, src, skip, 8, q)
            host = {"what": "the reference's cdef_filter_fb + compute_cdef_dist (C functions of libsvtref.so, -O2 -mavx2) driven from Python, "
                            "one host thread, 1080p 8-bit, window 0 .. 64, nothing skipped", "s": round(time.perf_counter() - t0, 3)}
            print(json.dumps(host), flush=True)
    res = {"tool": "tools/bench_cdef.py", "device": dsp.device_name(), "windows": nwin, "min_window_s": 0.2, "base_qindex": q,
           "method": "HIP events round windows of back-to-back calls, median", "rows": rows, "host_reference_1080p": host,
           "kernels": kernel_resources()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
