"""GPU: svt_hip_dlf_mi_frame / svt_hip_dlf_apply_frame / svt_hip_dlf_search_frame against the reference.  tests/golden/dlf.npz holds,
per case, the picture av1_loop_filter_frame left and the ss_err table of every plane and level (written by
tests/golden/make_golden_dlf.py from the reference's own EbDeblockingFilter.c), and the sixteen filters' outputs on edge units.
Every comparison is an equality."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dlf_cases as dc      # noqa: E402
import layouts            # noqa: E402
import poison               # noqa: E402
from poison import poisoned_outputs  # noqa: E402,F401

CASES = dc.case_names()


def dev(a, pad=0, fill=0):
    """numpy plane -> device tensor (uint16 travels as int16 bits), optionally with `pad` extra columns and rows of `fill`"""
    a = np.ascontiguousarray(a)
    if pad:
        b = np.full((a.shape[0] + pad, a.shape[1] + pad), fill, a.dtype)
        b[:a.shape[0], :a.shape[1]] = a
        a = b
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def host(t, like):
    a = t.cpu().numpy()
    return a.view(np.uint16) if like.dtype == np.uint16 else a


def call_args(c):
    row = c["row"]
    kw = dict(sharpness=int(row[dc.P_SHARP]))
    if row[dc.P_DELTA]:
        kw.update(ref_deltas=[int(v) for v in row[dc.P_RD:dc.P_RD + 8]], mode_deltas=[int(v) for v in row[dc.P_MD:dc.P_MD + 2]])
    return int(row[dc.P_W]), int(row[dc.P_H]), int(row[dc.P_BD]), [int(v) for v in row[dc.P_L0:dc.P_L0 + 4]], kw


def check_planes(got, want, w, h, fill=None, what=""):
    for i, (g, wnt) in enumerate(zip(got, want)):
        pw, ph = (w, h) if i == 0 else (w // 2, h // 2)
        a = host(g, wnt)
        bad = np.argwhere(a[:ph, :pw] != wnt)
        assert bad.size == 0, (what, i, len(bad), bad[:5], [(int(a[tuple(b)]), int(wnt[tuple(b)])) for b in bad[:5]])
        if fill is not None:
            assert (a[ph:] == fill).all() and (a[:, pw:] == fill).all(), (what, i, "a sample outside the picture was written")


@pytest.mark.parametrize("name", CASES)
def test_apply_equals_the_reference_picture_in_place_and_into_a_second_buffer(dsp, name):
    """both forms, with planes padded by 8 columns and rows of a fill value that must survive"""
    c = dc.case(name)
    w, h, bd, levels, kw = call_args(c)
    mi = torch.from_numpy(c["mi"]).cuda()
    rec = tuple(dev(p, 8, 201) for p in c["rec"])
    dst = tuple(torch.full_like(r, 93) for r in rec)
    dsp.dlf_apply_frame(rec, mi, w, h, bd, levels, dst=dst, **kw)
    torch.cuda.synchronize()
    check_planes(dst, c["out"], w, h, 93, "two buffers")
    check_planes(rec, c["rec"], w, h, 201, "the input of the two-buffer form")
    dsp.dlf_apply_frame(rec, mi, w, h, bd, levels, in_place=True, **kw)
    torch.cuda.synchronize()
    check_planes(rec, c["out"], w, h, 201, "in place")


@pytest.mark.parametrize("name", ["edge_mixed", "hbd_delta"])
def test_apply_into_planes_the_wrapper_allocates(dsp, name):
    c = dc.case(name)
    w, h, bd, levels, kw = call_args(c)
    dst = dsp.dlf_apply_frame(tuple(dev(p) for p in c["rec"]), torch.from_numpy(c["mi"]).cuda(), w, h, bd, levels, **kw)
    torch.cuda.synchronize()
    check_planes(dst, c["out"], w, h, None, "wrapper-allocated")


@pytest.mark.parametrize("name", ["sb1_mixed", "edge_mixed", "wide_delta", "hbd_mixed"])
def test_grid_built_from_the_final_list(dsp, name):
    """svt_hip_dlf_mi_frame on the case's final list gives the case's grid; entries that are left out (no source, a source past nsrc,
    reaching outside the grid) leave a sentinel untouched; apply on the built grid equals apply on the given one"""
    c = dc.case(name)
    w, h, bd, levels, kw = call_args(c)
    final, count, info = torch.from_numpy(c["final"].view(np.int32)).cuda(), torch.from_numpy(c["final_count"].view(np.int32)).cuda(), torch.from_numpy(c["info"]).cuda()
    mi = torch.full((h // 4 + 3, w // 4 + 5, 4), 0xEE, dtype=torch.uint8, device="cuda")
    dsp.dlf_mi_frame(final, count, info, mi, mi_cols=w // 4, mi_rows=h // 4)
    torch.cuda.synchronize()
    got = mi.cpu().numpy()
    assert np.array_equal(got[:h // 4, :w // 4], c["mi"])
    assert (got[h // 4:] == 0xEE).all() and (got[:, w // 4:] == 0xEE).all()
    out = dsp.dlf_apply_frame(tuple(dev(p) for p in c["rec"]), mi, w, h, bd, levels, **kw)
    torch.cuda.synchronize()
    check_planes(out, c["out"], w, h, None, "apply on the built grid")
    # left out: entry 0 of superblock 0 without a source, entry 1 with a source at nsrc, and a grid one unit too small for the last column
    f2 = c["final"].copy()
    f2[0, 0, 2] = dc.NO_SRC
    if c["final_count"][0] > 1:
        f2[0, 1, 2] = len(c["info"])
    mi2 = torch.full((h // 4, w // 4, 4), 0xEE, dtype=torch.uint8, device="cuda")
    dsp.dlf_mi_frame(torch.from_numpy(f2.view(np.int32)).cuda(), count, info, mi2, mi_cols=w // 4 - 1, mi_rows=h // 4)
    torch.cuda.synchronize()
    want = c["mi"].copy()
    for sb in range(len(c["final_count"])):
        for k in range(int(c["final_count"][sb])):
            w0, w1, src = (int(v) for v in f2[sb, k])
            x, y, bsize = w0 >> 16, w1 & 0xFFFF, w1 >> 16 & 255
            if src >= len(c["info"]) or (x + dc.BS_W[bsize]) // 4 > w // 4 - 1:
                want[y // 4:(y + dc.BS_H[bsize]) // 4, x // 4:(x + dc.BS_W[bsize]) // 4] = 0xEE
    want[:, w // 4 - 1] = 0xEE
    assert np.array_equal(mi2.cpu().numpy(), want)


@pytest.mark.parametrize("name", CASES)
def test_search_table_equals_the_reference(dsp, name):
    """all 64 levels, a 3-level mask and an empty mask; the reconstruction is unchanged after a search"""
    c = dc.case(name)
    w, h, bd, levels, kw = call_args(c)
    mi = torch.from_numpy(c["mi"]).cuda()
    rec, src = tuple(dev(p, 8, 201) for p in c["rec"]), tuple(dev(p, 8, 77) for p in c["src"])
    want = c["sse"].astype(np.uint64)
    got = dsp.dlf_search_frame(rec, src, mi, w, h, bd, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want), name
    masks = (1 << 0 | 1 << 7 | 1 << 33, 1 << 2 | 1 << 20 | 1 << 63, 1 << 1 | 1 << 12 | 1 << 40)
    want3 = np.full((3, 64), np.iinfo(np.uint64).max, np.uint64)
    for pl in range(3):
        for l in range(64):
            if masks[pl] >> l & 1:
                want3[pl, l] = want[pl, l]
    got3 = dsp.dlf_search_frame(rec, src, mi, w, h, bd, masks=masks, **kw)
    none = dsp.dlf_search_frame(rec, src, mi, w, h, bd, masks=(0, 0, 0), **kw)
    torch.cuda.synchronize()
    assert np.array_equal(got3.cpu().numpy().view(np.uint64), want3)
    assert (none.cpu().numpy() == -1).all()
    check_planes(rec, c["rec"], w, h, 201, "the reconstruction after a search")


@pytest.mark.parametrize("name", ["edge_mixed", "hbd_delta"])
def test_search_equals_the_sse_of_the_apply(dsp, name):
    """three levels: the table entry is the plain SSE of svt_hip_dlf_apply_frame's output at that level"""
    c = dc.case(name)
    w, h, bd, _, kw = call_args(c)
    mi = torch.from_numpy(c["mi"]).cuda()
    rec, src = tuple(dev(p) for p in c["rec"]), tuple(dev(p) for p in c["src"])
    tab = dsp.dlf_search_frame(rec, src, mi, w, h, bd, masks=(1 << 5 | 1 << 18 | 1 << 47,) * 3, **kw).cpu().numpy()
    for level in (5, 18, 47):
        out = dsp.dlf_apply_frame(rec, mi, w, h, bd, (level, level, level, level), **kw)
        for pl in range(3):
            a = host(out[pl], c["rec"][pl]).astype(np.int64)
            assert int(((a - c["src"][pl].astype(np.int64)) ** 2).sum()) == int(tab[pl, level]), (name, level, pl)


def test_stack_of_two_pictures_captured_into_a_graph(dsp):
    """apply (into a second buffer) and search on a stack of two pictures of one geometry, captured once and replayed twice: the same
    bytes each time; picture 0 equals the reference, picture 1 (another picture and grid under the same parameters) the same calls on
    it alone"""
    a, b = dc.case("sb1_mixed"), dc.case("sb1_allskip")
    w, h, bd, levels, kw = call_args(a)
    rec = tuple(torch.stack([dev(c["rec"][i]) for c in (a, b)]) for i in range(3))
    src = tuple(torch.stack([dev(c["src"][i]) for c in (a, b)]) for i in range(3))
    mi = torch.stack([torch.from_numpy(a["mi"]).cuda(), torch.from_numpy(b["mi"]).cuda()])
    alone = dsp.dlf_apply_frame(tuple(r[1].contiguous() for r in rec), mi[1].contiguous(), w, h, bd, levels, **kw)
    alone_sse = dsp.dlf_search_frame(tuple(r[1].contiguous() for r in rec), tuple(r[1].contiguous() for r in src), mi[1].contiguous(), w, h, bd, **kw)
    dst = tuple(torch.zeros_like(r) for r in rec)
    sse = torch.zeros((2, 3, 64), dtype=torch.int64, device="cuda")
    scratch = torch.zeros((dsp.dlf_search_scratch_bytes(w, h, 2),), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            dsp.dlf_apply_frame(rec, mi, w, h, bd, levels, dst=dst, **kw)
            dsp.dlf_search_frame(rec, src, mi, w, h, bd, sse=sse, scratch=scratch, **kw)
    results = []
    for _ in range(2):
        for t in dst + (sse,):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        results.append([t.cpu().numpy().copy() for t in dst + (sse,)])
    for x, y in zip(*results):
        assert np.array_equal(x, y)
    check_planes([d[0] for d in dst], a["out"], w, h, None, "picture 0 of the stack")
    assert np.array_equal(results[0][3][0].view(np.uint64), a["sse"])
    for i in range(3):
        assert torch.equal(dst[i][1], alone[i]), i
    assert torch.equal(sse[1], alone_sse)
    assert not torch.equal(sse[0], sse[1])


@pytest.mark.parametrize("name", ["edge_mixed", "hbd_delta"])
def test_apply_and_search_with_every_operand_laid_out_differently_equal_the_reference(dsp, name, poisoned_outputs):
    """rec / dst (apply into a second buffer) and rec / src (search): a stride per plane and role that no other plane of the call has, the
    chroma strides unrelated to luma's, mi_stride above mi_cols; alone, and as a stack of two (the fixture's picture second) with a pitch
    per plane, role and grid.  tests/layouts.py asserts the layouts distinct and a mix-up of them harmless before anything is uploaded."""
    c = dc.case(name)
    w, h, bd, levels, kw = call_args(c)
    fill = poisoned_outputs.fill_byte
    for n in (1, 2):
        pics = (lambda p: np.stack([np.ascontiguousarray(p[::-1, ::-1]), p])) if n == 2 else (lambda p: p)
        mi_np = np.stack([c["mi"], c["mi"]]) if n == 2 else c["mi"]
        spec = layouts.dlf_spec("svt_hip_dlf_apply_frame", w, h, ("rec", "dst"), n)
        lay = layouts.distinct_layouts(spec)
        assert lay["mi"].stride > w // 4
        rec, p_rec = layouts.place_operand(spec, lay, "rec", [pics(p) for p in c["rec"]], n, fill)
        dst, p_dst = layouts.place_operand(spec, lay, "dst", [layouts.poison_like(pics(p), fill) for p in c["rec"]], n, fill)
        mi, p_mi = layouts.place_operand(spec, lay, "mi", [mi_np], n, fill, record=True)
        dsp.dlf_apply_frame(rec, mi[0], w, h, bd, levels, dst=dst, **kw)
        torch.cuda.synchronize()
        check_planes([d[-1] if n == 2 else d for d in dst], c["out"], w, h, None, ("apply", n))
        layouts.assert_all_intact(p_rec + p_mi, fill)
        layouts.assert_all_intact(p_dst, fill, written=True)

        spec = layouts.dlf_spec("svt_hip_dlf_search_frame", w, h, ("rec", "src"), n)
        lay = layouts.distinct_layouts(spec)
        rec, p_rec = layouts.place_operand(spec, lay, "rec", [pics(p) for p in c["rec"]], n, fill)
        src, p_src = layouts.place_operand(spec, lay, "src", [pics(p) for p in c["src"]], n, fill)
        mi, p_mi = layouts.place_operand(spec, lay, "mi", [mi_np], n, fill, record=True)
        got = dsp.dlf_search_frame(rec, src, mi[0], w, h, bd, **kw)
        torch.cuda.synchronize()
        got = got.cpu().numpy().view(np.uint64).reshape(n, 3, 64)[-1]
        assert np.array_equal(got, c["sse"].astype(np.uint64)), ("search", n, np.argwhere(got != c["sse"].astype(np.uint64))[:4].tolist())
        layouts.assert_all_intact(p_rec + p_src + p_mi, fill)


def test_deblock_then_cdef_without_a_host_copy(dsp):
    """svt_hip_cdef_search_frame on the device-deblocked planes equals the same call on the fixture's deblocked planes"""
    c = dc.case("edge_mixed")
    w, h, bd, levels, kw = call_args(c)
    mi = torch.from_numpy(c["mi"]).cuda()
    src = tuple(dev(p) for p in c["src"])
    skip = torch.from_numpy(np.ascontiguousarray((c["mi"][::2, ::2, 2] >> 7) & (c["mi"][1::2, 1::2, 2] >> 7)).astype(np.uint8)).cuda()
    deblocked = dsp.dlf_apply_frame(tuple(dev(p) for p in c["rec"]), mi, w, h, bd, levels, **kw)
    got = dsp.cdef_search_frame(deblocked, src, skip, w, h, bd, 100)
    want = dsp.cdef_search_frame(tuple(dev(p) for p in c["out"]), src, skip, w, h, bd, 100)
    torch.cuda.synchronize()
    poison.assert_written(got, want)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert int(got[1].sum()) > 0


@pytest.mark.parametrize("bd", [8, 10])
def test_a_grid_of_random_bytes_writes_nothing_outside_the_picture(dsp, bd):
    rng = np.random.default_rng(7)
    w, h = 200, 136
    mi = torch.from_numpy(rng.integers(0, 256, (h // 4, w // 4, 4), dtype=np.uint8)).cuda()
    dt = np.uint8 if bd == 8 else np.uint16
    planes = [rng.integers(0, 1 << bd, (h >> (i > 0), w >> (i > 0))).astype(dt) for i in range(3)]
    rec = tuple(dev(p, 8, 201) for p in planes)
    dst = tuple(torch.full_like(r, 93) for r in rec)
    dsp.dlf_apply_frame(rec, mi, w, h, bd, (63, 40, 50, 33), sharpness=2, ref_deltas=[5, -7, 9, 0, -63, 63, 1, -1], mode_deltas=[4, -4], dst=dst)
    dsp.dlf_apply_frame(rec, mi, w, h, bd, (63, 40, 50, 33), sharpness=2, ref_deltas=[5, -7, 9, 0, -63, 63, 1, -1], mode_deltas=[4, -4], in_place=True)
    sse = dsp.dlf_search_frame(rec, dst, mi, w, h, bd, masks=(1 << 9 | 1 << 63,) * 3)
    torch.cuda.synchronize()
    for i, (r, d) in enumerate(zip(rec, dst)):
        pw, ph = w >> (i > 0), h >> (i > 0)
        for t, fill in ((r, 201), (d, 93)):
            a = host(t, planes[i])
            assert (a[ph:] == fill).all() and (a[:, pw:] == fill).all(), (i, fill)
    assert (sse.cpu().numpy()[:, [9, 63]] >= 0).all()


def test_the_sixteen_filters_on_edge_units(dsp):
    """The fixture's edge units, each as a small picture of two blocks (or rows of blocks) whose common edge has the wanted length and
    whose level and sharpness give the unit's recorded thresholds.  Compared: the samples the filter may modify (2, 2, 3, 6 per side
    for 4, 6, 8, 14), which no other edge of the pass touches."""
    g = dc.fixture()
    reach = {4: 2, 6: 2, 8: 3, 14: 6}
    luma_block = {(0, 4): 16, (1, 4): 17, (0, 8): 4, (1, 8): 5, (0, 14): 6, (1, 14): 6}      # 4x16, 16x4, 8x16, 16x8, 16x16
    thresholds = {}
    for sharp in (0, 3, 7):
        for level in range(1, 64):
            lim = level >> ((sharp > 0) + (sharp > 4))
            lim = max(min(lim, 9 - sharp) if sharp else lim, 1)
            thresholds.setdefault((2 * (level + 2) + lim, lim, level >> 4), (level, sharp))
    checked = 0
    for b, bd in enumerate((8, 10)):
        dt = np.uint8 if bd == 8 else np.uint16
        for dirn in range(2):
            for li, length in enumerate((4, 6, 8, 14)):
                chroma = length == 6
                units, par, want = g["filt_in"][b, dirn, li], g["filt_par"][b, dirn, li], g["filt_out"][b, dirn, li]
                for i in range(0, len(units), 3):
                    level, sharp = thresholds[tuple(int(v) for v in par[i])]
                    # luma 32x16 (vertical edge) or 16x32; for the 6-tap 32x32 luma blocks, whose chroma transform is 16x16, in 64x32
                    bsize, scale = (9, 2) if chroma else (luma_block[(dirn, length)], 1)
                    pic_w, pic_h = (32 * scale, 16 * scale) if dirn == 0 else (16 * scale, 32 * scale)
                    mi = np.zeros((pic_h // 4, pic_w // 4, 4), np.uint8)
                    mi[:, :] = (bsize, dc.tx_of(dc.BS_W[bsize], dc.BS_H[bsize]), 0, 0)
                    planes = [np.full((pic_h >> (k > 0), pic_w >> (k > 0)), 1 << (bd - 1), dt) for k in range(3)]
                    target = planes[1 if chroma else 0]
                    line = units[i].astype(dt)                                   # [4][16], the edge between columns 7 and 8
                    full = np.concatenate([np.repeat(line[:, :1], 8, 1), line, np.repeat(line[:, -1:], 8, 1)], 1)      # 32 across
                    tile = np.tile(full, (4, 1))                                 # [16][32]
                    target[:, :] = tile if dirn == 0 else tile.T
                    out = dsp.dlf_apply_frame(tuple(dev(p) for p in planes), torch.from_numpy(mi).cuda(), pic_w, pic_h, bd, (level,) * 4, sharpness=sharp)
                    torch.cuda.synchronize()
                    a = host(out[1 if chroma else 0], target)
                    a = a if dirn == 0 else a.T
                    r = reach[length]
                    got, exp = a[:4, 16 - r:16 + r], want[i][:, 8 - r:8 + r]
                    assert np.array_equal(got, exp), (bd, dirn, length, level, sharp, got.tolist(), exp.tolist())
                    checked += 1
    assert checked == 2 * 2 * 4 * 16


poison.add_second_fill(globals())
