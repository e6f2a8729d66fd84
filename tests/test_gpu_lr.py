"""GPU: svt_hip_lr_apply_frame / svt_hip_lr_try_frame / svt_hip_lr_wiener_stats_frame against the reference.  tests/golden/lr.npz
holds, per case, the picture the reference's loop restoration left, the squared error of trial filters per unit and the Wiener
statistics per unit, search_wiener_seg's outcome per unit and rest_finish_search's per plane (written by tests/golden/make_golden_lr.py from the reference's own
EbRestoration.c / EbRestorationPick.c).
Every comparison is an equality."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lr_cases as lc       # noqa: E402
import layouts            # noqa: E402
import poison               # noqa: E402
from poison import poisoned_outputs  # noqa: E402,F401

CASES = lc.case_names()


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


def check_planes(got, want, w, h, fill=None, what=""):
    for i, (g, wnt) in enumerate(zip(got, want)):
        pw, ph = (w, h) if i == 0 else (w // 2, h // 2)
        a = host(g, wnt)
        bad = np.argwhere(a[:ph, :pw] != wnt)
        assert bad.size == 0, (what, i, len(bad), bad[:5], [(int(a[tuple(b)]), int(wnt[tuple(b)])) for b in bad[:5]])
        if fill is not None:
            assert (a[ph:] == fill).all() and (a[:, pw:] == fill).all(), (what, i, "a sample outside the picture was written")


def geometry(c):
    return c["w"], c["h"], c["bd"], c["unit_size"]


@pytest.mark.parametrize("name", CASES)
def test_apply_equals_the_reference_picture(dsp, name):
    """planes padded by 8 columns and rows of a fill value that must survive, in the output and in both inputs"""
    c = lc.case(name)
    w, h, bd, us = geometry(c)
    cdef, dblk = tuple(dev(p, 8, 201) for p in c["cdef"]), tuple(dev(p, 8, 55) for p in c["dblk"])
    dst = tuple(torch.full_like(r, 93) for r in cdef)
    dsp.lr_apply_frame(cdef, dblk, w, h, bd, us, c["frame_type"], c["units"], dst=dst)
    torch.cuda.synchronize()
    check_planes(dst, c["out"], w, h, 93, "the restored picture")
    check_planes(cdef, c["cdef"], w, h, 201, "the CDEF picture after the call")
    check_planes(dblk, c["dblk"], w, h, 55, "the deblocked picture after the call")


@pytest.mark.parametrize("name", ["u64", "hbd"])
def test_apply_into_planes_the_wrapper_allocates_and_all_none_is_a_copy(dsp, name):
    c = lc.case(name)
    w, h, bd, us = geometry(c)
    cdef, dblk = tuple(dev(p) for p in c["cdef"]), tuple(dev(p) for p in c["dblk"])
    dst = dsp.lr_apply_frame(cdef, dblk, w, h, bd, us, c["frame_type"], c["units"])
    copy = dsp.lr_apply_frame(cdef, dblk, w, h, bd, us, (0, 0, 0), c["units"])
    torch.cuda.synchronize()
    check_planes(dst, c["out"], w, h, None, "wrapper-allocated")
    check_planes(copy, c["cdef"], w, h, None, "frame type none on every plane")


@pytest.mark.parametrize("name", CASES)
def test_try_equals_the_recorded_sse(dsp, name):
    """all of the case's candidates in one call (several per unit), then the same list reversed with one candidate out of range"""
    c = lc.case(name)
    w, h, bd, us = geometry(c)
    cdef, dblk, src = (tuple(dev(p, 8, f) for p in c[k]) for k, f in (("cdef", 201), ("dblk", 55), ("src", 77)))
    got = dsp.lr_try_frame(cdef, dblk, src, w, h, bd, us, c["cands"])
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    bad = np.argwhere(got != c["sse"])
    assert bad.size == 0, (name, len(bad), [(c["cands"][int(b)].tolist(), int(got[int(b)]), int(c["sse"][int(b)])) for b in bad[:4]])
    rev = c["cands"][::-1].copy()
    rev[1]["unit"] = 10000
    got = dsp.lr_try_frame(cdef, dblk, src, w, h, bd, us, rev).cpu().numpy()
    want = c["sse"][::-1].copy()
    want[1] = np.iinfo(np.int64).max
    assert np.array_equal(got, want)
    check_planes(cdef, c["cdef"], w, h, 201, "the CDEF picture after a try")


@pytest.mark.parametrize("name", ["u64", "hbd"])
def test_try_equals_the_sse_of_the_apply(dsp, name):
    """every unit under its own record of the case: the try's figure is the plain SSE of svt_hip_lr_apply_frame's output over the unit"""
    c = lc.case(name)
    w, h, bd, us = geometry(c)
    cdef, dblk, src = (tuple(dev(p) for p in c[k]) for k in ("cdef", "dblk", "src"))
    out = dsp.lr_apply_frame(cdef, dblk, w, h, bd, us, (3, 3, 3), c["units"])
    cands = np.zeros(c["offsets"][3], lc.CAND_DTYPE)
    for plane in range(3):
        for k in range(c["offsets"][plane + 1] - c["offsets"][plane]):
            i = c["offsets"][plane] + k
            cands[i]["plane"], cands[i]["unit"], cands[i]["u"] = plane, k, c["units"][i]
    sse = dsp.lr_try_frame(cdef, dblk, src, w, h, bd, us, cands).cpu().numpy()
    for i, cd in enumerate(cands):
        plane = int(cd["plane"])
        hs, he, vs, ve = lc.unit_limits(w, h, us, plane, int(cd["unit"]))
        a = host(out[plane], c["src"][plane]).astype(np.int64)[vs:ve, hs:he]
        assert int(((a - c["src"][plane][vs:ve, hs:he].astype(np.int64)) ** 2).sum()) == int(sse[i]), (name, i)


@pytest.mark.parametrize("name", CASES)
def test_statistics_equal_the_reference_per_unit_and_window(dsp, name):
    c = lc.case(name)
    w, h, bd, us = geometry(c)
    cdef, src = tuple(dev(p, 8, 201) for p in c["cdef"]), tuple(dev(p, 8, 77) for p in c["src"])
    M, H = dsp.lr_wiener_stats_frame(cdef, src, w, h, bd, us, c["win"])
    torch.cuda.synchronize()
    M, H = M.cpu().numpy(), H.cpu().numpy()
    for u in range(c["offsets"][3]):
        win, m, hh = lc.unpack_stats(c, u)
        w2 = win * win
        assert np.array_equal(M[u, :w2], m), (name, u, "M")
        assert np.array_equal(H[u, :w2 * w2].reshape(w2, w2), hh), (name, u, "H", np.argwhere(H[u, :w2 * w2].reshape(w2, w2) != hh)[:4].tolist())
        assert (M[u, w2:] == 0).all() and (H[u, w2 * w2:] == 0).all()


@pytest.mark.parametrize("name", CASES)
def test_wiener_search_equals_search_wiener_seg_per_unit(dsp, name):
    """dsp.lr_wiener_search (statistics on the device, derivation on the host, the walks of all units in lock step with one
    svt_hip_lr_try_frame per round) gives the reference's final taps and SSE for every unit, INT64_MAX where compute_score refuses; the
    rounds are the longest walk's trials"""
    c = lc.case(name)
    w, h, bd, us = geometry(c)
    cdef, dblk, src = (tuple(dev(p) for p in c[k]) for k in ("cdef", "dblk", "src"))
    taps, sse, rounds = dsp.lr_wiener_search(cdef, dblk, src, w, h, bd, us, c["win"])
    assert np.array_equal(sse, c["ws_sse"]), (name, np.argwhere(sse != c["ws_sse"])[:4].tolist())
    assert np.array_equal(taps, c["ws_final"]), (name, np.argwhere(taps != c["ws_final"])[:4].tolist())
    assert rounds == int(c["ws_n"].max())


@pytest.mark.parametrize("name", CASES)
def test_search_and_finish_equal_rest_finish_search_per_plane(dsp, name):
    """the unfiltered units' errors and the errors of the recorded self-guided parameters from svt_hip_lr_try_frame, the Wiener results
    from dsp.lr_wiener_search, then svt_hip_lr_finish per plane under every recorded setting: the reference's frame type and unit records;
    and the picture restored under the first setting's decision equals the plain model's"""
    c = lc.case(name)
    w, h, bd, us = geometry(c)
    cdef, dblk, src = (tuple(dev(p) for p in c[k]) for k in ("cdef", "dblk", "src"))
    n = c["offsets"][3]
    taps, wsse, _ = dsp.lr_wiener_search(cdef, dblk, src, w, h, bd, us, c["win"])
    cands = np.zeros(2 * n, lc.CAND_DTYPE)
    for plane in range(3):
        for k in range(c["offsets"][plane + 1] - c["offsets"][plane]):
            u = c["offsets"][plane] + k
            for i in (u, n + u):
                cands[i]["plane"], cands[i]["unit"] = plane, k
            cands[n + u]["u"]["type"], cands[n + u]["u"]["ep"], cands[n + u]["u"]["xqd"] = 2, c["results"][u]["ep"], c["results"][u]["xqd"]
    sse = dsp.lr_try_frame(cdef, dblk, src, w, h, bd, us, cands).cpu().numpy()
    res = np.zeros(n, lc.RESULT_DTYPE)
    res["sse"][:, 0], res["sse"][:, 1], res["sse"][:, 2] = sse[:n], wsse, sse[n:]
    res["vfilter"], res["hfilter"], res["ep"], res["xqd"] = taps[:, :3], taps[:, 3:], c["results"]["ep"], c["results"]["xqd"]
    assert np.array_equal(res["sse"], c["results"]["sse"]), (name, np.argwhere(res["sse"] != c["results"]["sse"])[:4].tolist())
    decided = None
    for i, (costs, row) in enumerate(zip(c["finishes"], c["fin_types"])):
        types, units = [], []
        for plane in range(3):
            a, b = c["offsets"][plane], c["offsets"][plane + 1]
            ft, un = dsp.lr_finish(plane, int(row[0]), costs, res[a:b], dsp.lib)
            types.append(ft); units.append(un)
            want = c["fin_units"][i][a:b]
            assert ft == int(row[1 + plane]), (name, i, plane)
            assert [int(v) for v in un["type"]] == [int(v) for v in want["type"]], (name, i, plane)
            for g_, w_ in zip(un, want):
                assert (g_["vfilter"].tolist(), g_["hfilter"].tolist()) == (w_["vfilter"].tolist(), w_["hfilter"].tolist()) if int(w_["type"]) == 1 else \
                    (int(g_["ep"]), g_["xqd"].tolist()) == (int(w_["ep"]), w_["xqd"].tolist()), (name, i, plane)
        decided = decided or (types, np.concatenate(units))
    out = dsp.lr_apply_frame(cdef, dblk, w, h, bd, us, decided[0], decided[1])
    m = dict(c)
    m["frame_type"], m["units"] = decided
    check_planes(out, lc.model_apply(m), w, h, None, "the picture under the finish's decision")


def test_stack_of_two_pictures_captured_into_a_graph(dsp):
    """apply, try and statistics on a stack of two pictures of one geometry, captured once and replayed twice: the same bytes each
    time; picture 0 equals the reference, picture 1 (the picture turned round, under the same records) the same calls on it alone"""
    c = lc.case("u64")
    w, h, bd, us = geometry(c)
    turn = lambda p: np.ascontiguousarray(p[::-1, ::-1])
    stack = lambda key: tuple(torch.stack([dev(p), dev(turn(p))]) for p in c[key])
    cdef, dblk, src = stack("cdef"), stack("dblk"), stack("src")
    units = np.concatenate([c["units"], c["units"]])
    cands = np.concatenate([c["cands"], c["cands"]])
    cands["pic"][len(c["cands"]):] = 1
    one = lambda planes: tuple(p[1].contiguous() for p in planes)
    alone = dsp.lr_apply_frame(one(cdef), one(dblk), w, h, bd, us, c["frame_type"], c["units"])
    alone_sse = dsp.lr_try_frame(one(cdef), one(dblk), one(src), w, h, bd, us, c["cands"])
    alone_m, alone_h = dsp.lr_wiener_stats_frame(one(cdef), one(src), w, h, bd, us, c["win"])
    dst = tuple(torch.zeros_like(r) for r in cdef)
    sse = torch.zeros((len(cands),), dtype=torch.int64, device="cuda")
    M = torch.zeros((2, c["offsets"][3], 49), dtype=torch.int64, device="cuda")
    H = torch.zeros((2, c["offsets"][3], 2401), dtype=torch.int64, device="cuda")
    scratch = torch.zeros((dsp.lr_stats_scratch_bytes(w, h, us, 2),), dtype=torch.uint8, device="cuda")
    d_units = dsp._lr_records(units, dsp.LR_UNIT_DTYPE, "cuda")
    d_cands = dsp._lr_records(cands, dsp.LR_CAND_DTYPE, "cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            dsp.lr_apply_frame(cdef, dblk, w, h, bd, us, c["frame_type"], d_units, dst=dst)
            dsp.lr_try_frame(cdef, dblk, src, w, h, bd, us, d_cands, sse=sse)
            dsp.lr_wiener_stats_frame(cdef, src, w, h, bd, us, c["win"], M=M, H=H, scratch=scratch)
    results = []
    for _ in range(2):
        for t in dst + (sse, M, H):
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        results.append([t.cpu().numpy().copy() for t in dst + (sse, M, H)])
    for x, y in zip(*results):
        assert np.array_equal(x, y)
    check_planes([d[0] for d in dst], c["out"], w, h, None, "picture 0 of the stack")
    n = len(c["cands"])
    assert np.array_equal(results[0][3][:n], c["sse"])
    for i in range(3):
        assert torch.equal(dst[i][1], alone[i]), i
    assert torch.equal(sse[n:], alone_sse) and torch.equal(M[1], alone_m) and torch.equal(H[1], alone_h)
    assert not torch.equal(sse[:n], sse[n:]) and not torch.equal(M[0], M[1])


@pytest.mark.parametrize("name", ["u64", "hbd"])
def test_every_operand_laid_out_differently_equals_the_reference(dsp, name, poisoned_outputs):
    """cdef / dblk / dst (apply), cdef / dblk / src (try) and cdef / src (statistics): a stride per plane and role that no other plane of
    the call has, the chroma strides unrelated to luma's; alone, and as a stack of two (the fixture's picture second) with a pitch per
    plane and role.  tests/layouts.py asserts the layouts distinct and a mix-up of them harmless before anything is uploaded."""
    c = lc.case(name)
    w, h, bd, us = geometry(c)
    fill = poisoned_outputs.fill_byte
    for n in (1, 2):
        pics = (lambda p: np.stack([np.ascontiguousarray(p[::-1, ::-1]), p])) if n == 2 else (lambda p: p)
        units = np.concatenate([c["units"]] * n)
        cands = np.concatenate([c["cands"]] * n)
        if n == 2:
            cands["pic"][len(c["cands"]):] = 1
        spec = layouts.picture_spec("svt_hip_lr_apply_frame", w, h, ("cdef", "dblk", "dst"), n)
        lay = layouts.distinct_layouts(spec)
        cdef, p_cdef = layouts.place_operand(spec, lay, "cdef", [pics(p) for p in c["cdef"]], n, fill)
        dblk, p_dblk = layouts.place_operand(spec, lay, "dblk", [pics(p) for p in c["dblk"]], n, fill)
        dst, p_dst = layouts.place_operand(spec, lay, "dst", [layouts.poison_like(pics(p), fill) for p in c["cdef"]], n, fill)
        dsp.lr_apply_frame(cdef, dblk, w, h, bd, us, c["frame_type"], units, dst=dst)
        torch.cuda.synchronize()
        check_planes([d[-1] if n == 2 else d for d in dst], c["out"], w, h, None, ("apply", n))
        layouts.assert_all_intact(p_cdef + p_dblk, fill)
        layouts.assert_all_intact(p_dst, fill, written=True)

        spec = layouts.picture_spec("svt_hip_lr_try_frame", w, h, ("cdef", "dblk", "src"), n)
        lay = layouts.distinct_layouts(spec)
        cdef, p_cdef = layouts.place_operand(spec, lay, "cdef", [pics(p) for p in c["cdef"]], n, fill)
        dblk, p_dblk = layouts.place_operand(spec, lay, "dblk", [pics(p) for p in c["dblk"]], n, fill)
        src, p_src = layouts.place_operand(spec, lay, "src", [pics(p) for p in c["src"]], n, fill)
        got = dsp.lr_try_frame(cdef, dblk, src, w, h, bd, us, cands).cpu().numpy()
        assert np.array_equal(got[-len(c["cands"]):], c["sse"]), ("try", n)
        layouts.assert_all_intact(p_cdef + p_dblk + p_src, fill)

        spec = layouts.picture_spec("svt_hip_lr_wiener_stats_frame", w, h, ("cdef", "src"), n)
        lay = layouts.distinct_layouts(spec)
        cdef, p_cdef = layouts.place_operand(spec, lay, "cdef", [pics(p) for p in c["cdef"]], n, fill)
        src, p_src = layouts.place_operand(spec, lay, "src", [pics(p) for p in c["src"]], n, fill)
        M, H = dsp.lr_wiener_stats_frame(cdef, src, w, h, bd, us, c["win"])
        M, H = M.cpu().numpy().reshape(n, -1, 49)[-1], H.cpu().numpy().reshape(n, -1, 2401)[-1]
        for u in (0, c["offsets"][1], c["offsets"][3] - 1):
            win, m, hh = lc.unpack_stats(c, u)
            assert np.array_equal(M[u, :win * win], m) and np.array_equal(H[u, :win ** 4].reshape(win * win, win * win), hh), ("statistics", n, u)
        layouts.assert_all_intact(p_cdef + p_src, fill)


def test_cdef_then_restoration_without_a_host_copy(dsp):
    """the fixture's chain case carries the skip map, the strengths and base_qindex under which the reference's CDEF made its CDEF
    picture of its deblocked one: svt_hip_cdef_apply_frame on the deblocked planes gives that picture, and svt_hip_lr_apply_frame on the
    planes it left on the device (the deblocked planes as stripe context) gives the reference's restored picture"""
    c = lc.case("chain")
    g = lc.fixture()
    w, h, bd, us = geometry(c)
    skip = torch.from_numpy(np.ascontiguousarray(g["c200_skip"])).cuda()
    luma, chroma = torch.from_numpy(np.ascontiguousarray(g["c200_ystr"])).cuda(), torch.from_numpy(np.ascontiguousarray(g["c200_ustr"])).cuda()
    dblk = tuple(dev(p) for p in c["dblk"])
    cdef = dsp.cdef_apply_frame(dblk, skip, luma, chroma, w, h, bd, int(g["c200_qindex"]))
    got = dsp.lr_apply_frame(cdef, dblk, w, h, bd, us, c["frame_type"], c["units"])
    torch.cuda.synchronize()
    check_planes(cdef, c["cdef"], w, h, None, "the device's CDEF picture")
    check_planes(got, c["out"], w, h, None, "restoration of the device's CDEF picture")
    for i in range(3):
        assert not torch.equal(cdef[i], dblk[i]) and not torch.equal(got[i], cdef[i]), i


@pytest.mark.parametrize("bd", [8, 10])
def test_records_of_random_bytes_write_nothing_outside_the_picture(dsp, bd):
    rng = np.random.default_rng(7)
    w, h, us = 200, 136, (64, 32, 32)
    dt = np.uint8 if bd == 8 else np.uint16
    planes = [rng.integers(0, 1 << bd, (h >> (i > 0), w >> (i > 0))).astype(dt) for i in range(3)]
    _, per_pic = dsp.lr_unit_grid(w, h, us)
    units = torch.from_numpy(rng.integers(0, 256, per_pic * 24, dtype=np.uint8)).cuda()
    cands = rng.integers(0, 256, 40 * 36, dtype=np.uint8).view(lc.CAND_DTYPE).copy()
    cands["pic"][:30], cands["plane"][:30], cands["unit"][:30] = 0, rng.integers(0, 3, 30), rng.integers(0, 6, 30)
    cdef, dblk = tuple(dev(p, 8, 201) for p in planes), tuple(dev(p[::-1].copy(), 8, 55) for p in planes)
    dst = tuple(torch.full_like(r, 93) for r in cdef)
    dsp.lr_apply_frame(cdef, dblk, w, h, bd, us, (3, 3, 3), units, dst=dst)
    sse = dsp.lr_try_frame(cdef, dblk, dst, w, h, bd, us, cands)
    torch.cuda.synchronize()
    for i, (r, b, d) in enumerate(zip(cdef, dblk, dst)):
        pw, ph = w >> (i > 0), h >> (i > 0)
        for t, fill in ((r, 201), (b, 55), (d, 93)):
            a = host(t, planes[i])
            assert (a[ph:] == fill).all() and (a[:, pw:] == fill).all(), (i, fill)
        assert int(host(d, planes[i])[:ph, :pw].max()) < (1 << bd)
    assert (sse.cpu().numpy()[:30] >= 0).all()


poison.add_second_fill(globals())
