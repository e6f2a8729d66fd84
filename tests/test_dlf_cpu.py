"""CPU: the deblocking calls' host side.  csrc/dlf_plan.h as a stand-alone program (tests/c/dlf_plan_host.cpp), built plain and under
AddressSanitizer + UBSan and run directly; the host helpers of the level pick against the reference's own runs recorded in
tests/golden/dlf.npz (av1_pick_filter_level whole, both branches; LPF_PICK_FROM_Q over every qindex); the limit and level tables; the
fixture's coverage facts; the argument checks through the C ABI, which need no device; and, where oracle/_ref/libsvtref_dlf.so is
present, one case re-run live against the fixture."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cidana-svt-av1_amd")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dlf_cases as dc  # noqa: E402

ERR_INVALID = -2
MIN_COVER = 20


@pytest.mark.parametrize("san_flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_dlf_plan(tmp_path, san_flags):
    """every clause of dlf_check / dlf_search_check / dlf_mi_check refuses its one changed field and accepts the neighbour of each bound;
    the limit, level, side and length tables equal closed forms; the scratch size; the walk on synthetic tables, whole and in rounds"""
    exe = str(tmp_path / "dlf_plan_host")
    pr = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror"] + san_flags +
                        [os.path.join(ROOT, "tests", "c", "dlf_plan_host.cpp"), os.path.join(PKG, "csrc", "host_err.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip() == "ok"


def test_walk_equals_av1_pick_filter_level(pkg):
    """the helper's walk over the recorded table chooses what av1_pick_filter_level(LPF_PICK_FROM_FULL_IMAGE) chose: luma starts at the
    previous filter_level_u (dir is 2 there), Cb at the previous u, Cr at the previous v; filling the table in NEED_LEVEL rounds
    converges to the same level and asks for no level twice"""
    g = dc.fixture()
    pics = [str(s) for s in g["walk_pics"]]
    seen = set()
    for lfm, only4, l0, l1, lu, lv, w0, w1, wu, wv, sharp, pic in g["walks"].tolist():
        table = g[f"walk_table_{pics[pic]}_{sharp}"].astype(np.int64)
        for plane, start, want in ((0, lu, w0), (1, lu, wu), (2, lv, wv)):
            assert pkg.SvtHipDsp.dlf_pick_level(table[plane], start, lfm, only4) == ("level", want), (lfm, only4, start, plane)
            lazy, asked = np.full(64, -1, np.int64), []
            while True:
                kind, level = pkg.SvtHipDsp.dlf_pick_level(lazy, start, lfm, only4)
                if kind == "level":
                    break
                assert lazy[level] < 0 and level not in asked
                asked.append(level)
                lazy[level] = table[plane, level]
            assert level == want and 1 <= len(asked) <= (3 if lfm <= 2 else 64)
        assert w0 == w1
        seen.add((lfm <= 2, only4))
    assert seen == {(True, 0), (True, 1), (False, 0), (False, 1)}


def test_level_from_q_equals_the_reference(pkg):
    g = dc.fixture()
    for b, bd in enumerate((8, 10)):
        for key in (0, 1):
            for q in range(256):
                assert pkg.SvtHipDsp.dlf_level_from_q(q, bd, key) == g["from_q"][b, key, q].tolist(), (bd, key, q)
    lib = pkg.load_library()
    lv = (ctypes.c_int * 4)()
    assert lib.svt_hip_dlf_level_from_q(256, 8, 0, lv) == ERR_INVALID and lib.svt_hip_dlf_level_from_q(-1, 8, 0, lv) == ERR_INVALID
    assert lib.svt_hip_dlf_level_from_q(10, 9, 0, lv) == ERR_INVALID and lib.svt_hip_dlf_level_from_q(10, 8, 0, None) == ERR_INVALID


def test_limit_and_level_tables(pkg):
    """svt_hip_dlf_limits gives the thresholds the fixture's filter units were recorded with; svt_hip_dlf_levels equals the model the
    generator counted its coverage with, for every case"""
    lib = pkg.load_library()
    g = dc.fixture()
    want = {tuple(int(v) for v in p) for p in g["filt_par"].reshape(-1, 3)}
    have = set()
    out = (ctypes.c_uint8 * 3)()
    for sharp in range(8):
        for level in range(64):
            assert lib.svt_hip_dlf_limits(level, sharp, out) == 0
            lim, mblim, hev = out[1 - 1], out[1], out[2]
            assert mblim == 2 * (level + 2) + lim and hev == level >> 4 and 1 <= lim <= (63 if sharp == 0 else 9 - sharp)
            have.add((mblim, lim, hev))
    assert want <= have
    assert lib.svt_hip_dlf_limits(64, 0, out) == ERR_INVALID and lib.svt_hip_dlf_limits(0, 8, out) == ERR_INVALID
    for name in dc.case_names():
        row = dc.case(name)["row"]
        kw = {}
        if row[dc.P_DELTA]:
            kw = dict(ref_deltas=row[dc.P_RD:dc.P_RD + 8], mode_deltas=row[dc.P_MD:dc.P_MD + 2])
        p = _host_pic(pkg, row, **kw)
        tab = np.zeros((3, 2, 8, 2), np.uint8)
        assert lib.svt_hip_dlf_levels(ctypes.addressof(p), tab.ctypes.data) == 0
        for plane in range(3):
            for dirn in range(2):
                for ref in range(8):
                    for mode in (0, 13, 15, 16, 24):
                        if (ref == 0) == (mode < 13):
                            assert tab[plane, dirn, ref, dc.MODE_LF[mode]] == dc.unit_level(row, plane, dirn, ref, mode), (name, plane, dirn, ref, mode)


def test_fixture_coverage(pkg):
    """what the generator asserted from the reference's output, as stored"""
    g = dc.fixture()
    edges, lines = g["cover_edges"], g["cover_lines"]
    for dirn in range(2):
        assert all(edges[0, dirn, n] >= MIN_COVER for n in (4, 8, 14)) and all(edges[1, dirn, n] >= MIN_COVER for n in (4, 6))
        assert (lines[dirn, 14] >= MIN_COVER).all() and (lines[dirn, 8, :3] >= MIN_COVER).all() and (lines[dirn, 4, :2] >= MIN_COVER).all()
    assert int(g["cover_pv_level"]) >= MIN_COVER
    fl = g["cover_filter_lines"]
    for b in range(2):
        for dirn in range(2):
            for li, top in enumerate((1, 1, 2, 3)):
                assert (fl[b, dirn, li, :top + 1] >= MIN_COVER).all(), (b, dirn, li)
    names = dc.case_names()
    rows = [dc.case(n)["row"] for n in names]
    assert {(int(r[dc.P_W]), int(r[dc.P_H]), int(r[dc.P_BD])) for r in rows} == {(64, 64, 8), (200, 136, 8), (328, 200, 8), (72, 72, 10)}
    assert {int(r[dc.P_SHARP]) for r in rows} == {0, 3, 7}
    assert any(r[dc.P_L0] == 0 and r[dc.P_L1] == 0 and r[dc.P_LU] and r[dc.P_LV] for r in rows)        # the gating quirk
    assert any(r[dc.P_L0] != r[dc.P_L1] and r[dc.P_L0] and r[dc.P_L1] for r in rows)
    assert any(r[dc.P_DELTA] for r in rows)
    skip = dc.case("sb1_allskip")["mi"]
    assert ((skip[:, :, 2] >> 7) == 1).all() and ((skip[:, :, 2] & 7) > 0).all()
    sizes = set()
    for n in names:
        sizes |= set(np.unique(dc.case(n)["mi"][:, :, 0]).tolist())
    assert sizes == set(range(13)) | set(range(16, 22))                                               # every block size but the 128-wide ones


def _host_pic(pkg, row, planes=None, ref_deltas=None, mode_deltas=None, in_place=False):
    """a svt_hip_dlf_pic over host addresses (nothing dereferences them)"""
    import torch
    w, h, bd = int(row[dc.P_W]), int(row[dc.P_H]), int(row[dc.P_BD])
    dt = torch.uint8 if bd == 8 else torch.int16
    mk = lambda: tuple(torch.zeros((h >> (i > 0), w >> (i > 0)), dtype=dt) for i in range(3))
    rec, src = mk(), mk()
    dst = rec if in_place else mk()
    mi = torch.zeros((h // 4, w // 4, 4), dtype=torch.uint8)
    p = pkg.SvtHipDsp.make_dlf_pic(rec, mi, w, h, bd, [int(v) for v in row[dc.P_L0:dc.P_L0 + 4]], int(row[dc.P_SHARP]),
                                   None if ref_deltas is None else [int(v) for v in ref_deltas], None if mode_deltas is None else [int(v) for v in mode_deltas],
                                   src=src, dst=dst)
    p._keep = (rec, src, dst, mi)
    return p


def test_argument_checks_through_the_c_abi(pkg):
    """svt_hip_dlf_check / svt_hip_dlf_mi_check / svt_hip_dlf_search_scratch_bytes run without a device"""
    lib = pkg.load_library()
    row = dc.case("edge_mixed")["row"]
    for in_place in (False, True):
        for search in (0, 1):
            assert lib.svt_hip_dlf_check(ctypes.addressof(_host_pic(pkg, row, in_place=in_place)), search) == 0, lib.svt_hip_last_error()

    def refused(search, **change):
        p = _host_pic(pkg, row)
        for k, v in change.items():
            if isinstance(v, tuple):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return lib.svt_hip_dlf_check(ctypes.addressof(p), search) == ERR_INVALID

    assert lib.svt_hip_dlf_check(None, 0) == ERR_INVALID
    for search in (0, 1):
        assert refused(search, d_rec=(1, None)) and refused(search, d_mi=None)
        assert refused(search, width=204) and refused(search, height=132) and refused(search, width=65536)
        assert refused(search, rec_stride=(0, 199)) and refused(search, mi_stride=49)
        assert refused(search, sharpness_level=8) and refused(search, bit_depth=12)
        assert refused(search, ref_deltas=(7, 64)) and refused(search, mode_deltas=(1, -64)) and refused(search, npics=0)
    assert refused(0, filter_level=(1, 64)) and refused(0, filter_level_u=64) and refused(0, filter_level_v=-1)
    assert refused(0, d_dst=(2, None)) and refused(1, d_src=(0, None))
    p = _host_pic(pkg, row)
    p.d_dst[0] = p.d_rec[0]                            # one plane in place, two not
    assert lib.svt_hip_dlf_check(ctypes.addressof(p), 0) == ERR_INVALID
    p = _host_pic(pkg, row)
    p.d_dst[1] = p.d_rec[1] + 16                       # overlapping without being equal
    assert lib.svt_hip_dlf_check(ctypes.addressof(p), 0) == ERR_INVALID
    assert lib.svt_hip_dlf_search_scratch_bytes(200, 136, 2) == 4 * 3 * 2 * 3 * 64 * 8 and lib.svt_hip_dlf_search_scratch_bytes(204, 136, 1) == 0
    a = pkg.SvtHipDsp.DlfMiArgs()
    buf = np.zeros(4096, np.uint8)
    a.d_final = a.d_final_count = a.d_info = a.d_mi = buf.ctypes.data
    a.npics, a.nsb, a.nsrc, a.mi_cols, a.mi_rows, a.mi_stride = 1, 12, 100, 50, 34, 50
    assert lib.svt_hip_dlf_mi_check(ctypes.addressof(a)) == 0
    for field, bad in (("d_info", None), ("nsb", 0), ("nsrc", 0), ("mi_stride", 49), ("mi_rows", 0), ("sb_pitch", 11), ("mi_cols", 16385)):
        b = pkg.SvtHipDsp.DlfMiArgs.from_buffer_copy(a)
        setattr(b, field, bad)
        assert lib.svt_hip_dlf_mi_check(ctypes.addressof(b)) == ERR_INVALID, field
    assert lib.svt_hip_dlf_mi_check(None) == ERR_INVALID


@pytest.mark.skipif(dc.ref_dlf() is None, reason="oracle/_ref/libsvtref_dlf.so is built by tests/golden/make_golden_dlf.py, where the reference is")
def test_live_reference_equals_the_fixture():
    c = dc.case("hbd_delta")
    out = dc.ref_frame(c["row"], c["rec"], c["mi"])
    for got, want in zip(out, c["out"]):
        assert np.array_equal(got, want)
    assert np.array_equal(dc.ref_table(c["row"], c["rec"], c["src"], c["mi"]), c["sse"])
    assert sorted(n for n, _, _, _ in dc.edge_units(c["row"], c["mi"], 0, 0))      # the model runs on the case
