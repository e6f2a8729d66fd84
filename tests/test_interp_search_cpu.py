"""CPU: the golden fixture of the interpolation filter search (tests/golden/interp_search.npz, written by
tests/golden/make_golden_interp_search.py: the leaves are the reference's compiled convolve entries, highbd_variance64_c and
model_rd_from_sse, the glue is the generator's, see there), the numpy walk against it and, where the reference is built, the leaves
again; the C ABI of the three calls and the size query as the header declares it and the Python mirror binds it."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "interp_search.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_inter_pred as mg  # noqa: E402
import make_golden_interp_search as ms  # noqa: E402

HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libsvtref.so"))
INVALID, NO_DEVICE = -2, -1


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def test_fixture_loads_and_meets_the_conditions(gold):
    """every shape x direction with the four corners on the clamp, all phase classes in luma and chroma, tail workgroups, a block whose
    nine totals are zero; in FULL every pair wins somewhere and DUAL_FAST differs somewhere; the synthetic ties, both ends of the
    model's table and a rate term past 2^32"""
    tabs = ms.model_tables()
    assert np.array_equal(np.stack(tabs), gold["model_tabs"])
    st = ms.check_conditions(gold, tabs)
    assert st["winners"] == 9 and st["differ"] > 0 and st["tie0"] and st["tie_vertical"] and st["big_rate"] and st["xsq_max"] and st["xsq_zero"]
    assert int(gold["planes_crc"][0]) == mg.planes_crc(mg.planes_of(8, "random"))
    assert os.path.getsize(GOLD) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "inter_pred.npz"))
    assert ms.FILTER_SETS == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]
    assert [ms.pair_filters(i) for i in (0, 1, 3, 8)] == [0, 1 << 16, 1, 2 | 2 << 16]              # filter_sets[i][0] is the VERTICAL filter


def test_the_numpy_restatement_regenerates_the_fixture(gold):
    """predictions by make_golden_inter_pred's numpy restatement, SSE and walk by this generator's glue"""
    taps = np.load(os.path.join(ROOT, "tests", "golden", "inter_pred.npz"))["taps"]
    planes = mg.planes_of(8, "random")
    z = ms.generate(lambda ss, p, bw, bh, blk: mg.np_inter_pred(taps, planes, 8, ss, p, bw, bh, blk), ms.np_sse, ms.np_model_of(ms.model_tables()))
    assert sorted(list(z) + ["model_tabs"]) == sorted(gold)
    for k, v in z.items():
        assert v.dtype == gold[k].dtype and np.array_equal(v, gold[k]), k


def test_hand_computed_walks():
    """a table with no model in it (lambda 0 leaves dist * 128; the model is the identity here) so that the order of the walk is all
    that decides"""
    model_of = lambda bw, bh: (lambda s, p, q: (0, s))
    rates = np.zeros((16, 3), np.int32)

    def run(row, mode, searchable=1, lam=0, use_uv=0):
        sse = np.array([row, row, row], np.uint32)
        return ms.walk(model_of(8, 8), sse, [0, 0], searchable, 8, 8, use_uv, lam, 400, rates, mode)

    row = [50, 60, 40, 45, 10, 70, 45, 5, 70]
    assert run(row, ms.FULL)[0] == ms.pair_filters(7)                                     # the global minimum
    assert run(row, ms.DUAL_FAST)[0] == ms.pair_filters(2)                                # pair 2 wins the first three; its column is 5, 8
    assert run([50, 40, 60, 45, 10, 70, 45, 10, 70], ms.DUAL_FAST)[0] == ms.pair_filters(4)      # 4 and 7 tie: the first stays
    assert run(row, ms.SINGLE)[0] == ms.pair_filters(4)                                   # 0, 4, 8 only
    assert run(row, ms.FULL, searchable=0)[:3] == (0, 0, 50 * 128)
    assert run([7] * 9, ms.FULL) == (0, 0, 7 * 128, 7 << 4, 0) and run([0] * 9, ms.FULL) == (0, 0, 0, 0, 1)
    assert run([7] * 9, ms.FULL, use_uv=1) == (0, 0, 21 * 128, 21 << 4, 0)
    # the rate: dir 0 reads the vertical filter's row entry, dir 1 the horizontal one's
    rates[3] = (100, 200, 300)
    rates[9] = (1, 2, 3)
    assert [ms.switchable_rate(rates, [3, 9], i) for i in (0, 1, 3, 8)] == [101, 102, 201, 303]
    assert ms.rdcost(512, 3, 5) == 3 + 640 and ms.rdcost(1, 255, 0) == 0 and ms.rdcost(1, 256, 0) == 1
    assert ms.rdcost(1, -1, 0) == (((1 << 64) - 1 + 256) & ms.M64) >> 9                    # (uint64_t)(R) of a negative int


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/libsvtref.so is built from the reference tree, which is not on this machine")
def test_the_reference_leaves_again_on_random_cases(gold):
    R = ms.ref_lib()
    assert R is not None
    tabs = ms.model_tables()
    rng = np.random.default_rng(0x1EAF)
    for _ in range(400):                                        # model_rd_from_sse over its whole domain
        (w, h), bsize = list(ms.BSIZE.items())[int(rng.integers(0, len(ms.BSIZE)))]
        sse = int(rng.choice((0, 1, 2, int(rng.integers(0, 1 << 12)), int(rng.integers(0, 1 << 24)), int(rng.integers(0, 1 << 32)), 0xFFFFFFFF)))
        q = int(rng.choice((0, 4, 8, int(rng.integers(0, 1 << 8)), int(rng.integers(0, 1 << 15)), 32767)))
        assert ms.ref_model_rd(R, bsize, q, sse) == ms.np_model_rd(tabs, sse, (w * h).bit_length() - 1, q), (w, h, sse, q)
    for _ in range(300):                                        # highbd_variance64_c
        w, h = int(rng.choice((4, 8, 16, 32, 64))), int(rng.choice((4, 8, 16, 32, 64)))
        a, b = rng.integers(0, 256, (h, w)).astype(np.uint8), rng.integers(0, 256, (h, w)).astype(np.uint8)
        if rng.integers(0, 4) == 0:
            a[:], b[:] = 255, 0
        assert ms.ref_sse(R, a, b) == ms.np_sse(a, b)
    planes = mg.planes_of(8, "random")
    for gi in (0, 5, 8, 16):                                    # the SSE tables through the compiled convolve entries
        bw, bh, d, same = (int(v) for v in gold["groups"][gi])
        blk = ms.blocks_of(gold, gi)[:6]
        got = ms.sse_table(lambda ss, p, w_, h_, b_: mg.ref_inter_pred(R, planes, 8, ss, p, w_, h_, b_), lambda x, y: ms.ref_sse(R, x, y), planes, bw, bh, blk, same)
        assert np.array_equal(got, gold[f"sse_{gi}"][:6]), gi


def test_header_declares_the_entries_and_the_mirror_binds_them(pkg):
    hdr = open(os.path.join(ROOT, "include", "svt_hip_dsp.h")).read()
    for decl in ("int svt_hip_interp_sse_frame(const svt_hip_interp_sse_group *groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd,",
                 "int svt_hip_interp_decide_frame(const svt_hip_interp_decide_group *groups, int ngroups, const svt_hip_interp_params *params, void *stream);",
                 "size_t svt_hip_interp_search_scratch_bytes(const svt_hip_interp_search_group *groups, int ngroups, int use_uv);",
                 "int svt_hip_interp_search_frame(const svt_hip_interp_search_group *groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd,"):
        assert decl in hdr, decl
    for cite in ("EbInterPrediction.c:3578-3917", ":3573", ":3231", ":3440-3529", ":3184", ":3305", ":3672-3825", ":3909-3911", "BORDER CONTRACT", "d_blk_out may equal"):
        assert cite in hdr, cite
    lib = pkg.load_library()
    for name, nargs, ret in (("svt_hip_interp_sse_frame", 7, ctypes.c_int), ("svt_hip_interp_decide_frame", 4, ctypes.c_int),
                             ("svt_hip_interp_search_scratch_bytes", 3, ctypes.c_size_t), ("svt_hip_interp_search_frame", 9, ctypes.c_int)):
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == nargs and f.restype is ret, name
    assert (pkg.INTERP_DUAL_FAST, pkg.INTERP_FULL, pkg.INTERP_SINGLE) == (ms.DUAL_FAST, ms.FULL, ms.SINGLE) == (0, 1, 2)
    assert "enum { SVT_HIP_INTERP_DUAL_FAST = 0, SVT_HIP_INTERP_FULL = 1, SVT_HIP_INTERP_SINGLE = 2 };" in hdr
    assert pkg.interp_decision_dtype() == ms.DEC_DTYPE and ctypes.sizeof(pkg.InterpDecision) == 32


def test_struct_layouts_match_the_header(pkg):
    structs = (("svt_hip_interp_sse_group", pkg.InterpSseGroup), ("svt_hip_interp_decision", pkg.InterpDecision), ("svt_hip_interp_params", pkg.InterpParams),
               ("svt_hip_interp_decide_group", pkg.InterpDecideGroup), ("svt_hip_interp_search_group", pkg.InterpSearchGroup))
    args, want = [], []
    for cname, S in structs:
        fields = [n for n, _ in S._fields_]
        args += [f"sizeof({cname})"] + [f"offsetof({cname}, {n})" for n in fields]
        want += [ctypes.sizeof(S)] + [getattr(S, n).offset for n in fields]
    code = ('#include <stddef.h>\n#include <stdio.h>\n#include "svt_hip_dsp.h"\nint main(void){printf("%zu"' + ' " %zu"' * (len(args) - 1) + ", " +
            ", ".join(args) + ");return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert out == want
    assert want[args.index("sizeof(svt_hip_interp_decision)")] == 32


def test_scratch_bytes_on_hand_computed_cases(pkg):
    """HOST: per non-empty group without a table of its own, nblocks * planes * 36 bytes rounded up to 16"""
    lib = pkg.load_library()

    def sb(specs, use_uv):
        arr = (pkg.InterpSearchGroup * max(len(specs), 1))()
        for a, (n, own) in zip(arr, specs):
            a.sse.nblocks, a.sse.bwidth, a.sse.bheight = n, 16, 16
            a.sse.d_sse = 0x1000 if own else None
        return lib.svt_hip_interp_search_scratch_bytes(arr, len(specs), use_uv)

    assert sb([(1, False)], 0) == 48 and sb([(1, False)], 1) == 112
    assert sb([(10, False), (0, False), (7, True), (33, False)], 1) == 1088 + 3568
    assert sb([(10, False), (0, False), (7, True), (33, False)], 0) == 368 + 1200
    assert sb([(7, True)], 1) == 0 and sb([], 1) == 0 and sb([(5, False)], 2) == 0
    assert lib.svt_hip_interp_search_scratch_bytes(None, 1, 1) == 0 and lib.svt_hip_interp_search_scratch_bytes(None, -1, 0) == 0


def test_the_calls_without_a_device_or_with_a_null_list(pkg):
    import torch
    lib = pkg.load_library()
    bad = INVALID if torch.cuda.is_available() else NO_DEVICE
    assert lib.svt_hip_interp_sse_frame(None, 1, 104, 72, 8, 1, None) == bad
    assert lib.svt_hip_interp_sse_frame(None, 1, 104, 72, 10, 1, None) == bad
    assert lib.svt_hip_interp_decide_frame(None, 1, None, None) == bad
    assert lib.svt_hip_interp_search_frame(None, 1, 104, 72, 8, None, None, 0, None) == bad


def test_the_kernels_are_in_the_built_library():
    """so that tests/test_kernel_resources.py, which holds every kernel of the library to no scratch, covers them"""
    data = open(os.path.join(ROOT, "cidana-svt-av1_amd", "libsvt_hip_dsp.so"), "rb").read()
    assert data.count(b"interp_sse_kernel") >= 2 and data.count(b"interp_decide_kernel") >= 2
    for sym in (b"svt_hip_interp_sse_frame", b"svt_hip_interp_decide_frame", b"svt_hip_interp_search_frame", b"svt_hip_interp_search_scratch_bytes"):
        assert sym in data
