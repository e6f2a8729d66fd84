"""CPU: the C-ABI library loads here (no GPU) and exports every symbol that
include/svt_hip_dsp.h declares; the host layer fails LOUDLY without a device (no
CPU fallback); the package never touches oracle/."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "svt_hip_dsp.h")
PKG = os.path.join(ROOT, "cidana-svt-av1_amd")


def declared_symbols():
    """every function the header declares, after preprocessing (most drop-ins come out of X-macro lists)"""
    txt = subprocess.check_output(["gcc", "-E", "-P", "-I", os.path.join(ROOT, "include"), HDR]).decode()
    return sorted(set(re.findall(r"\b(svt_hip_[a-z0-9_]+)\s*\(", txt)))


def test_library_loads_and_exports_every_declared_symbol(pkg):
    lib = pkg.load_library()
    names = declared_symbols()
    assert len(names) >= 540, len(names)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_header_compiles_as_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "svt_hip_dsp.h"\nint main(void){ svt_txfm_param p; (void)p; return sizeof(svt_hip_rtcd_table) > 0 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_txfm_param_layout_matches_reference():
    """TxfmParam is 24 bytes with eob at offset 20 (EbDefinitions.h:764-776)."""
    code = '#include <stddef.h>\n#include <stdio.h>\n#include "svt_hip_dsp.h"\nint main(void){printf("%zu %zu %zu", sizeof(svt_txfm_param), offsetof(svt_txfm_param, bd), offsetof(svt_txfm_param, eob));return 0;}\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(code)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    assert out == ["24", "8", "20"]


def test_no_device_is_a_loud_error_not_a_fallback(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.SvtHipError):
        pkg.SvtHipDsp(0)
    lib = pkg.load_library()
    rc = lib.svt_hip_fwd_txfm2d_batch(None, 8, 64, None, 1, 1, 0, 8, None)
    assert rc != 0 and lib.svt_hip_last_error()


def test_product_does_not_reference_the_oracle():
    """Nothing under the package (sources or the built .so) may import, link or name oracle/."""
    for dp, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp", ".c")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "svt_oracle" not in txt and "libsvt_oracle" not in txt and "libsvtref" not in txt, os.path.join(dp, f)
    so = os.path.join(PKG, "libsvt_hip_dsp.so")
    deps = subprocess.check_output(["ldd", so]).decode()
    assert "oracle" not in deps and "svtref" not in deps


def test_log_scale_rule(pkg):
    want = {0: 0, 1: 0, 2: 0, 3: 1, 4: 2, 9: 1, 10: 1, 11: 2, 12: 2, 15: 0, 17: 1, 18: 1}
    for s, ls in want.items():
        assert pkg.tx_log_scale(s) == ls


def test_host_tables_match_oracle():
    """cidana-svt-av1_amd/tables.py (what bench.py and the tools feed the quantiser with) against the oracle's
    av1_build_quantizer / scan restatements, which tests/test_oracle_golden.py (test_scan_tables, test_quantizer_tables:
    tests/golden/tables.npz = the reference's own arrays) pins to the reference."""
    import numpy as np
    import __graft_entry__ as ge
    import svtlibs
    pkg = ge.load_package()
    for bd in (8, 10, 12):
        a, b = pkg.tables.quant_tables(bd), svtlibs.quant_tables(bd)
        for k in b:
            assert np.array_equal(a[k], b[k]), (bd, k)
    for s in range(19):
        for t in range(16):
            if not svtlibs.txfm_allowed(s, t):
                continue
            sa, ia = pkg.tables.scan_tables(s, t)
            sb, ib = svtlibs.scan_tables(s, t)
            assert np.array_equal(sa, sb) and np.array_equal(ia, ib), (s, t)


# ---- round 2: slot registry, host tables behind the C ABI, a C caller ------------------------------------------------
EXPECTED_SLOTS = 19 + 19 + 1 + 6 + 1 + 10 * 19 * 2 + 2 + 6 + 4 + 1 + 2 + 1 + 22 * 2


def registry(lib):
    lib.svt_hip_rtcd_slot_name.restype = ctypes.c_char_p
    lib.svt_hip_rtcd_slot_function.restype = ctypes.c_void_p
    lib.svt_hip_rtcd_slot_function.argtypes = [ctypes.c_char_p]
    n = lib.svt_hip_rtcd_slot_count()
    return [lib.svt_hip_rtcd_slot_name(i).decode() for i in range(n)]


def test_slot_registry_is_complete_and_consistent(pkg):
    lib = pkg.load_library()
    names = registry(lib)
    assert len(names) == EXPECTED_SLOTS == len(set(names))
    assert lib.svt_hip_rtcd_slot_name(len(names)) is None and lib.svt_hip_rtcd_slot_name(-1) is None
    special = {"ResidualKernel": "svt_hip_residual_kernel"}
    for n in names:
        fn = lib.svt_hip_rtcd_slot_function(n.encode())
        sym = special.get(n, "svt_hip_" + n)
        assert fn and fn == ctypes.cast(getattr(lib, sym), ctypes.c_void_p).value, n
    assert lib.svt_hip_rtcd_slot_function(b"aom_variance16x16") is None
    slot = ctypes.c_void_p(0x1234)
    assert lib.svt_hip_rtcd_override_slot(b"no_such_slot", ctypes.byref(slot)) != 0 and slot.value == 0x1234


def test_slot_names_and_signatures_are_the_references(pkg):
    """every registry name is a dispatch global of the reference's aom_dsp_rtcd.h, and the drop-in's parameter list equals the
    reference's, token for token, after type-name normalisation (svtlibs.rtcd_param_types).  The reference's side is
    tests/golden/rtcd_slots.json: slot name -> parameter types, written by make_golden.py from the header (svtlibs.ref_slot_types)."""
    import json
    import svtlibs
    lib = pkg.load_library()
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "rtcd_slots.json")))
    hdr = subprocess.check_output(["gcc", "-E", "-P", "-I", os.path.join(ROOT, "include"), HDR]).decode()
    names = registry(lib)
    assert set(names) == set(ref)
    checked = 0
    for n in names:
        sym = "svt_hip_residual_kernel" if n == "ResidualKernel" else "svt_hip_" + n
        d = re.search(r"\b" + sym + r"\s*\(([^;]*)\)\s*;", hdr)
        assert d, sym
        assert ref[n] == svtlibs.rtcd_param_types(d.group(1)), (n, ref[n], svtlibs.rtcd_param_types(d.group(1)))
        checked += 1
    assert checked == EXPECTED_SLOTS


def test_host_tables_c_abi_equal_python_and_reference_arrays(pkg):
    """svt_hip_build_quantizer / svt_hip_get_scan / svt_hip_ois_candidates (csrc/host_tables.cpp) == tables.py ==
    the reference's own arrays (tests/golden/tables.npz, written by make_golden.py from av1_build_quantizer / av1_scan_orders)"""
    import numpy as np
    lib = pkg.load_library()
    g = np.load(os.path.join(ROOT, "tests", "golden", "tables.npz"))
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for bd in (8, 10, 12):
        t = {k: np.zeros((256, 8), np.int16) for k in ("zbin", "round", "quant", "quant_shift", "dequant")}
        assert lib.svt_hip_build_quantizer(bd, P(t["zbin"]), P(t["round"]), P(t["quant"]), P(t["quant_shift"]), P(t["dequant"])) == 0
        py = pkg.tables.quant_tables(bd)
        for k in t:
            assert np.array_equal(t[k], g[f"{k}_{bd}"]) and np.array_equal(t[k], py[k]), (k, bd)
    assert lib.svt_hip_build_quantizer(9, None, None, None, None, None) != 0
    for s in range(19):
        for ty in range(16):
            sc = np.zeros(1024, np.int16); isc = np.zeros(1024, np.int16)
            n = lib.svt_hip_get_scan(s, ty, P(sc), P(isc))
            assert n == len(g[f"scan_{s}_{ty}"])
            assert np.array_equal(sc[:n], g[f"scan_{s}_{ty}"]) and np.array_equal(isc[:n], g[f"iscan_{s}_{ty}"]), (s, ty)
    assert lib.svt_hip_get_scan(19, 0, None, None) < 0
    for bsize in (8, 16, 32, 64):
        for tl in (0, 1):
            for ipm in (0, 4, 5):
                for isref in (0, 1):
                    for is16 in (0, 1):
                        m = np.zeros(61, np.uint8); d = np.zeros(61, np.int8)
                        n = lib.svt_hip_ois_candidates(bsize, tl, ipm, isref, is16, P(m), P(d))
                        pm, pd = pkg.SvtHipDsp.ois_candidates(bsize, tl, ipm, bool(isref), bool(is16))
                        assert n == len(pm) and np.array_equal(m[:n], pm) and np.array_equal(d[:n], pd), (bsize, tl, ipm, isref, is16)


C_CALLER = os.path.join(ROOT, "tests", "c", "rtcd_caller.c")


def build_c_caller(tmp_path):
    exe = str(tmp_path / "rtcd_caller")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), C_CALLER, "-o", exe,
                           "-L", PKG, "-lsvt_hip_dsp", "-Wl,-rpath," + PKG])
    return exe


def test_c_caller_compiles_and_links_against_the_library(tmp_path):
    """a plain-C host (gcc, -lsvt_hip_dsp) that keeps its own block of dispatch pointers, as the reference does, lets the
    library fill them by name and calls through them; here it must build and, without a device, fail loudly"""
    import torch
    exe = build_c_caller(tmp_path)
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_dropin.py runs it")
    pr = subprocess.run([exe], capture_output=True, text=True)
    assert pr.returncode == 3, (pr.returncode, pr.stdout, pr.stderr)      # 3 = every override refused (no device), the host's own pointers intact and callable


def test_rtcd_override_refuses_without_a_device_and_leaves_the_pointers_alone(pkg):
    """SURVEY 8(b) "Errors": with no usable device svt_hip_rtcd_override / _override_slot return an error and do not touch the
    caller's dispatch pointers - the encoder keeps the AVX2 kernels setup_rtcd_internal already stored (its own fallback)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the override succeeds (tests/test_gpu_dropin.py)")
    lib = pkg.load_library()
    for name in registry(lib)[::37]:
        slot = ctypes.c_void_p(0x5a5a)
        rc = lib.svt_hip_rtcd_override_slot(name.encode(), ctypes.byref(slot))
        assert rc == -1 and slot.value == 0x5a5a, name                      # SVT_HIP_ERR_NO_DEVICE
    assert b"HIP device" in lib.svt_hip_last_error() or b"gfx950" in lib.svt_hip_last_error()
    # the table form: 19 + 19 + 8 pointer-to-pointer members (include/svt_hip_dsp.h, svt_hip_rtcd_table)
    nslots = 19 + 19 + 8
    store = (ctypes.c_void_p * nslots)(*([0x77] * nslots))
    table = (ctypes.c_void_p * nslots)(*[ctypes.addressof(store) + i * ctypes.sizeof(ctypes.c_void_p) for i in range(nslots)])
    assert lib.svt_hip_rtcd_override(ctypes.byref(table)) == -1
    assert all(v == 0x77 for v in store)


def test_intra_availability_host_helper_equals_reference_tables_and_oracle(pkg):
    """svt_hip_intra_has_top_right / _has_bottom_left (coding-order keys, csrc/host_tables.cpp) against every enumerated look-up of
    the reference's has_tr_* / has_bl_* tables (tests/golden/bip.npz), and svt_hip_intra_neighbor_px against the oracle's
    restatement of av1_predict_intra_block's availability half on the committed block cases and on random ones"""
    import numpy as np
    import svtlibs
    lib = pkg.load_library()
    g = np.load(os.path.join(ROOT, "tests", "golden", "bip.npz"))
    for sb_mi in (16, 32):
        n = int(g[f"avail_count_sb{sb_mi}"][0])
        tr = np.unpackbits(g[f"has_tr_sb{sb_mi}"])[:n]
        bl = np.unpackbits(g[f"has_bl_sb{sb_mi}"])[:n]
        i = 0
        for args in svtlibs.availability_tuples(sb_mi):
            assert lib.svt_hip_intra_has_top_right(sb_mi, *args) == tr[i], args
            assert lib.svt_hip_intra_has_bottom_left(sb_mi, *args) == bl[i], args
            i += 1
        assert i == n
    # arguments the reference asserts on are refused, not answered
    assert lib.svt_hip_intra_has_top_right(16, 0, 64, 96, 1, 1, 6, 0, 0, 0, 0, 0) < 0          # 4x4 has no VERT_A order
    assert lib.svt_hip_intra_has_top_right(24, 3, 64, 96, 1, 1, 0, 0, 0, 0, 0, 0) < 0
    O = svtlibs.oracle()
    H = pkg.SvtHipDsp.__new__(pkg.SvtHipDsp)          # host helpers only: no device
    H.lib = lib

    def product_px(c):
        pos = pkg.SvtHipDsp.IntraPos(c["is16"], 16, c["mi_rows"], c["mi_cols"], int(c["tile"][0]), int(c["tile"][1]), int(c["tile"][2]),
                                     int(c["tile"][3]), c["partition"], c["bsize"], c["tx"], c["plane"], c["micol"] * 4, c["mirow"] * 4,
                                     c["col_off"], c["row_off"], c["wpx"], c["hpx"])
        blk = pkg.SvtHipDsp.IntraBlk()
        assert lib.svt_hip_intra_neighbor_px(ctypes.addressof(pos), ctypes.addressof(blk)) == 0
        return [blk.n_top_px, blk.n_topright_px, blk.n_left_px, blk.n_bottomleft_px]

    cases = [c for c, _ in svtlibs.pib_fixture_cases(g)]
    rng = np.random.default_rng(77)
    for trial in range(4000):
        c = svtlibs.intra_block_case(rng, trial)
        if c is not None:
            cases.append(c)
    assert len(cases) > 3000
    for c in cases:
        _, out5 = svtlibs.oracle_predict_intra_block(O, c)
        assert product_px(c) == out5[:4].tolist(), {k: v for k, v in c.items() if np.isscalar(v)}


FRAME_HOST = os.path.join(ROOT, "tests", "c", "frame_host.c")


def build_frame_host(tmp_path):
    exe = str(tmp_path / "frame_host")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), FRAME_HOST, "-o", exe,
                           "-L", PKG, "-lsvt_hip_dsp", "-Wl,-rpath," + PKG])
    return exe


def test_c_frame_host_compiles_and_fails_loudly_without_a_device(tmp_path):
    """tests/c/frame_host.c: the batched interface driven from plain C (tables from the library's host builders, uploads, one
    svt_hip_encode_recon_frame call, digest); builds with gcc against the header and the library, and without a device exits 3"""
    import torch
    exe = build_frame_host(tmp_path)
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_frame_api.py runs it")
    pr = subprocess.run([exe, "128", "64", "100", "7"], capture_output=True, text=True)
    assert pr.returncode == 3, (pr.returncode, pr.stdout, pr.stderr)


def test_y4m_reader_host_side_equals_oracle_and_reference_fixture(pkg, tmp_path):
    """n4 host side (no device): svt_hip_y4m_parse_header accepts / rejects and parses as the oracle does (itself pinned to the
    reference application, picture.npz), and svt_hip_y4m_open / _read_frame / _close return a written file's frames"""
    import numpy as np
    import svtlibs
    lib = pkg.load_library()
    O = svtlibs.oracle()
    g = np.load(os.path.join(ROOT, "tests", "golden", "picture.npz"))
    for line, exp in zip(g["y4m_lines"].tolist(), g["y4m_out"].tolist()):
        oi = svtlibs.Y4mInfo()
        orc = O.svt_oracle_y4m_parse_header(line.encode(), ctypes.byref(oi))
        if orc != 0:
            with pytest.raises(pkg.SvtHipError):
                pkg.y4m_parse_header(lib, line)
            assert exp[1] != 0
            continue
        pi = pkg.y4m_parse_header(lib, line)
        for f in ("width", "height", "fr_n", "fr_d", "bit_depth", "interlaced", "chroma", "scan_type"):
            assert getattr(pi, f) == getattr(oi, f), (line, f)
        assert [pi.width, pi.height, pi.fr_n, pi.fr_d, pi.bit_depth, pi.interlaced] == exp[2:8]
    rng = np.random.default_rng(248)
    for trial in range(2000):                             # random headers: the product parser == the oracle's, field by field
        line = svtlibs.random_y4m_header(rng)
        oi = svtlibs.Y4mInfo()
        orc = O.svt_oracle_y4m_parse_header(line.encode(), ctypes.byref(oi))
        pi = pkg.Y4mInfo()
        prc = lib.svt_hip_y4m_parse_header(line.encode(), ctypes.addressof(pi))
        assert (orc == 0) == (prc == 0), line
        if orc == 0:
            for f in ("width", "height", "fr_n", "fr_d", "bit_depth", "interlaced", "chroma", "scan_type"):
                assert getattr(pi, f) == getattr(oi, f), (line, f)
    rng = np.random.default_rng(5)
    for bd, token in ((8, "C420jpeg"), (10, "C420p10")):
        w, h = 22, 10
        dt = np.uint8 if bd == 8 else np.dtype("<u2")
        frames = [(rng.integers(0, 1 << bd, (h, w)).astype(dt), rng.integers(0, 1 << bd, (h // 2, w // 2)).astype(dt),
                   rng.integers(0, 1 << bd, (h // 2, w // 2)).astype(dt)) for _ in range(3)]
        path = str(tmp_path / f"t{bd}.y4m")
        svtlibs.write_y4m(path, f" W{w} H{h} F30:1 Ip {token}\n", frames)
        with pkg.Y4mReader(lib, path) as rd:
            assert (rd.info.width, rd.info.height, rd.info.bit_depth) == (w, h, bd)
            assert rd.frame_bytes == (w * h + 2 * (w // 2) * (h // 2)) * dt.itemsize if bd > 8 else rd.frame_bytes == w * h * 3 // 2
            buf = np.zeros(rd.frame_bytes, np.uint8)
            for fr in frames:
                assert rd.read_into(buf)
                assert buf.tobytes() == b"".join(np.ascontiguousarray(p).tobytes() for p in fr)
            assert not rd.read_into(buf)                 # end of file
            with pytest.raises(pkg.SvtHipError):
                rd.read_into(np.zeros(4, np.uint8))      # too small a buffer is an error, not a short read
    # frames of 4 MiB and more are read by several threads (pread on disjoint ranges): same bytes, end of file and truncation as before
    w, h = 2048, 1536
    big = [tuple(rng.integers(0, 256, s).astype(np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))) for _ in range(2)]
    path = str(tmp_path / "big.y4m")
    svtlibs.write_y4m(path, f" W{w} H{h} F30:1 Ip C420jpeg\n", big)
    with pkg.Y4mReader(lib, path) as rd:
        buf = np.zeros(rd.frame_bytes, np.uint8)
        for fr in big:
            assert rd.read_into(buf) and buf.tobytes() == b"".join(p.tobytes() for p in fr)
        assert not rd.read_into(buf)
    os.truncate(path, os.path.getsize(path) - 1000)
    with pkg.Y4mReader(lib, path) as rd:
        assert rd.read_into(buf)
        with pytest.raises(pkg.SvtHipError):
            rd.read_into(buf)
    bad = str(tmp_path / "raw.yuv")
    open(bad, "wb").write(b"\x10" * 100)
    with pytest.raises(pkg.SvtHipError):
        pkg.Y4mReader(lib, bad)
    broken = str(tmp_path / "broken.y4m")
    open(broken, "wb").write(b"YUV4MPEG2 W4 H2 F1:1\nFRAMX\n" + b"\x00" * 12)
    with pkg.Y4mReader(lib, broken) as rd:
        with pytest.raises(pkg.SvtHipError):
            rd.read_into(np.zeros(rd.frame_bytes, np.uint8))


def test_committed_generated_headers_are_what_their_generators_emit(tmp_path):
    """csrc/gen/qlookup_gen.h == tools/gen_qlookup.py's output for qlookup_data.py (an edit to either must not leave the committed
    header, and with it the library's quantiser tables, behind; build.py regenerates on a newer generator, this catches the rest)"""
    import importlib.util
    import io
    import contextlib
    spec = importlib.util.spec_from_file_location("gen_qlookup", os.path.join(PKG, "tools", "gen_qlookup.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    out = str(tmp_path / "qlookup_gen.h")
    with contextlib.redirect_stdout(io.StringIO()):
        m.main(out)
    assert open(out).read() == open(os.path.join(PKG, "csrc", "gen", "qlookup_gen.h")).read()
