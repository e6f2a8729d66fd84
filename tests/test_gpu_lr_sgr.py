"""GPU: svt_hip_lr_sgr_stats_frame / svt_hip_lr_sgr_walk_frame / svt_hip_lr_sgr_search_frame against the reference.
tests/golden/lr_sgr.npz holds, per case and (unit, ep), what one round of search_selfguided_restoration's loop left (the projection's
start, every evaluation of the walk, the final xqd and its error) and per unit and ep range what search_sgrproj_seg left (ep, xqd, SSE),
written by tests/golden/make_golden_lr_sgr.py from the reference's own EbRestorationPick.c; the sums come from the plain model of
tests/lr_sgr_cases.py, which tests/test_lr_sgr_cpu.py ties to the reference's filtered planes and starts.
Every comparison is an equality.  The scratch is filled with a byte pattern before every call: nothing may depend on what it held."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lr_cases as lc       # noqa: E402
import lr_sgr_cases as sc   # noqa: E402
import layouts            # noqa: E402
from poison import poisoned_outputs  # noqa: E402,F401

CASES = sc.case_names()
PATTERN = 0xA5


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


def check_planes(got, want, w, h, fill=None, what=""):
    for i, (g, wnt) in enumerate(zip(got, want)):
        pw, ph = (w, h) if i == 0 else (w // 2, h // 2)
        a = g.cpu().numpy()
        a = a.view(np.uint16) if wnt.dtype == np.uint16 else a
        bad = np.argwhere(a[:ph, :pw] != wnt)
        assert bad.size == 0, (what, i, len(bad), bad[:5].tolist())
        if fill is not None:
            assert (a[ph:] == fill).all() and (a[:, pw:] == fill).all(), (what, i, "a sample outside the picture was written")


def scratch_for(dsp, c, npics=1, lo=0, hi=16):
    need = dsp.lr_sgr_scratch_bytes(c["w"], c["h"], c["unit_size"], npics, lo, hi)
    assert need > 0
    return torch.full((need,), PATTERN, dtype=torch.uint8, device="cuda")


def geometry(c):
    return c["w"], c["h"], c["bd"], c["unit_size"]


def model_sums(c):
    """[units, 16, 5] from the plain model"""
    out = np.zeros((c["offsets"][3], 16, 5), np.int64)
    for plane, k, u in sc.units_of(c):
        for ep in range(16):
            out[u, ep] = sc.sums(*sc.model(c, plane, k, ep))
    return out


def walk_records(t):
    return t.cpu().numpy().view(sc.WALK_DTYPE).reshape(t.shape[:-1])


def best_records(t):
    return t.cpu().numpy().view(sc.BEST_DTYPE).reshape(t.shape[:-1])


def check_walk(c, w, lo, hi, what):
    for f, want in (("start", c["start"]), ("xqd", c["final"]), ("err", c["err"]), ("evals", c["ntrials"])):
        bad = np.argwhere(w[f][:, lo:hi] != want[:, lo:hi])
        assert bad.size == 0, (c["name"], what, f, len(bad), bad[:4].tolist(), w[f][:, lo:hi][tuple(bad[0][:2])], want[:, lo:hi][tuple(bad[0][:2])])
    assert int(w["evals"].max()) <= sc.MAX_EVALS


@pytest.mark.parametrize("name", CASES)
def test_statistics_equal_the_model_s_sums_per_unit_and_ep(dsp, name):
    """all 16 ep, then a narrower range into a poisoned array: its entries are defined, the others untouched.  The planes are padded by 8
    columns and rows of a fill value that must survive."""
    c = sc.case(name)
    w, h, bd, us = geometry(c)
    cdef, src = tuple(dev(p, 8, 201) for p in c["cdef"]), tuple(dev(p, 8, 77) for p in c["src"])
    want = model_sums(c)
    stats = torch.full((c["offsets"][3], 16, 5), -3, dtype=torch.int64, device="cuda")
    dsp.lr_sgr_stats_frame(cdef, src, w, h, bd, us, 0, 16, stats=stats, scratch=scratch_for(dsp, c))
    torch.cuda.synchronize()
    got = stats.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    stats.fill_(-3)
    dsp.lr_sgr_stats_frame(cdef, src, w, h, bd, us, 9, 15, stats=stats, scratch=scratch_for(dsp, c, 1, 9, 15))
    got = stats.cpu().numpy()
    assert np.array_equal(got[:, 9:15], want[:, 9:15]) and (got[:, :9] == -3).all() and (got[:, 15:] == -3).all()
    check_planes(cdef, c["cdef"], w, h, 201, "the CDEF picture after the call")
    check_planes(src, c["src"], w, h, 77, "the source after the call")


@pytest.mark.parametrize("name", CASES)
def test_walk_equals_the_reference_s_start_result_and_evaluations(dsp, name):
    """d_start NULL: the start is solved on the device from the sums - it, the final xqd, the error and the number of evaluations are
    the reference's for every (unit, ep).  The same with the start given (svt_hip_lr_sgr_solve on the host, which is the recorded
    start), and with a start outside the ranges, which is clamped.  Then a narrower range on its own scratch."""
    c = sc.case(name)
    w, h, bd, us = geometry(c)
    cdef, src = tuple(dev(p) for p in c["cdef"]), tuple(dev(p) for p in c["src"])
    scratch = scratch_for(dsp, c)
    stats, _ = dsp.lr_sgr_stats_frame(cdef, src, w, h, bd, us, 0, 16, scratch=scratch)
    check_walk(c, walk_records(dsp.lr_sgr_walk_frame(cdef, src, w, h, bd, us, scratch, 0, 16, stats=stats)), 0, 16, "device solve")
    host = stats.cpu().numpy()
    start = np.zeros((c["offsets"][3], 16, 2), np.int16)
    for plane, k, u in sc.units_of(c):
        hs, he, vs, ve = lc.unit_limits(w, h, us, plane, k)
        for ep in range(16):
            start[u, ep] = dsp.lr_sgr_solve(host[u, ep], (he - hs) * (ve - vs), ep, dsp.lib)
    assert np.array_equal(start, c["start"])
    given = walk_records(dsp.lr_sgr_walk_frame(cdef, src, w, h, bd, us, scratch, 0, 16, start=torch.from_numpy(start).cuda()))
    check_walk(c, given, 0, 16, "start given")
    wild = start.astype(np.int32) + np.where(start >= np.array(sc.XQD_MAX), 1000, 0) - np.where(start <= np.array(sc.XQD_MIN), 1000, 0)
    check_walk(c, walk_records(dsp.lr_sgr_walk_frame(cdef, src, w, h, bd, us, scratch, 0, 16, start=torch.from_numpy(wild.astype(np.int16)).cuda())), 0, 16, "clamped")
    scratch = scratch_for(dsp, c, 1, 4, 12)
    stats, _ = dsp.lr_sgr_stats_frame(cdef, src, w, h, bd, us, 4, 12, scratch=scratch)
    part = walk_records(dsp.lr_sgr_walk_frame(cdef, src, w, h, bd, us, scratch, 4, 12, stats=stats))
    check_walk(c, part, 4, 12, "range 4 .. 12")
    assert not part.view(np.uint8).reshape(len(part), 16, -1)[:, :4].any() and not part.view(np.uint8).reshape(len(part), 16, -1)[:, 12:].any()


@pytest.mark.parametrize("name", CASES)
def test_search_equals_search_sgrproj_seg_per_unit_and_range(dsp, name):
    """the recorded settings - the full range, two mid +- step ranges and the empty one: ep, xqd and the SSE of
    try_restoration_unit_seg per unit; the projection error is the winning entry's (-1 for the empty range); the winners' histogram is
    sg_frame_ep_cnt.  The deblocked picture differs from the CDEF picture on every halo row of an inner stripe boundary (asserted on the
    fixture), so a search that filtered under the stripe rule, or a try that did not, would show."""
    c = sc.case(name)
    w, h, bd, us = geometry(c)
    cdef, dblk, src = (tuple(dev(p, 8, f) for p in c[k]) for k, f in (("cdef", 201), ("dblk", 55), ("src", 77)))
    for ri, (r0, r1, mode, lo, hi) in enumerate(sc.ranges()):
        a, b = dsp.lr_sgr_ep_range((r0, r1), mode, dsp.lib)
        assert (a, b) == (lo, hi) if lo >= 0 else a == b
        best = best_records(dsp.lr_sgr_search_frame(cdef, dblk, src, w, h, bd, us, a, b, scratch=scratch_for(dsp, c, 1, a, b)))
        want = c["search"][ri]
        for f, col in (("ep", want[:, 0]), ("sse", want[:, 3])):
            assert np.array_equal(best[f], col), (name, ri, f, np.argwhere(best[f] != col)[:4].tolist())
        assert np.array_equal(best["xqd"], want[:, 1:3]), (name, ri, np.argwhere(best["xqd"] != want[:, 1:3])[:4].tolist())
        proj = c["err"][np.arange(len(want)), want[:, 0]] if lo >= 0 else np.full(len(want), -1)
        assert np.array_equal(best["proj_err"], proj), (name, ri)
        assert np.array_equal(np.bincount(best["ep"], minlength=16), c["cnt"][ri])
    check_planes(cdef, c["cdef"], w, h, 201, "the CDEF picture after a search")
    check_planes(dblk, c["dblk"], w, h, 55, "the deblocked picture after a search")


@pytest.mark.parametrize("name", ["u64", "hbd"])
def test_every_operand_laid_out_differently_equals_the_reference(dsp, name, poisoned_outputs):
    """cdef / src (statistics, walk) and cdef / dblk / src (search): a stride per plane and role that no other plane of the call has,
    the chroma strides unrelated to luma's; alone, and as a stack of two (the fixture's picture second) with a pitch per plane and role.
    tests/layouts.py asserts the layouts distinct and a mix-up of them harmless before anything is uploaded."""
    c = sc.case(name)
    w, h, bd, us = geometry(c)
    fill = poisoned_outputs.fill_byte
    sums = model_sums(c)
    full = c["search"][0]
    for n in (1, 2):
        pics = (lambda p: np.stack([np.ascontiguousarray(p[::-1, ::-1]), p])) if n == 2 else (lambda p: p)
        spec = layouts.picture_spec("svt_hip_lr_sgr_stats_frame", w, h, ("cdef", "src"), n)
        lay = layouts.distinct_layouts(spec)
        cdef, p_cdef = layouts.place_operand(spec, lay, "cdef", [pics(p) for p in c["cdef"]], n, fill)
        src, p_src = layouts.place_operand(spec, lay, "src", [pics(p) for p in c["src"]], n, fill)
        scratch = scratch_for(dsp, c, n)
        stats, _ = dsp.lr_sgr_stats_frame(cdef, src, w, h, bd, us, 0, 16, scratch=scratch)
        walk = walk_records(dsp.lr_sgr_walk_frame(cdef, src, w, h, bd, us, scratch, 0, 16, stats=stats))
        assert np.array_equal(stats.cpu().numpy().reshape(n, -1, 16, 5)[-1], sums), ("statistics", n)
        check_walk(c, walk.reshape(n, -1, 16)[-1], 0, 16, ("walk", n))
        layouts.assert_all_intact(p_cdef + p_src, fill)

        spec = layouts.picture_spec("svt_hip_lr_sgr_search_frame", w, h, ("cdef", "dblk", "src"), n)
        lay = layouts.distinct_layouts(spec)
        cdef, p_cdef = layouts.place_operand(spec, lay, "cdef", [pics(p) for p in c["cdef"]], n, fill)
        dblk, p_dblk = layouts.place_operand(spec, lay, "dblk", [pics(p) for p in c["dblk"]], n, fill)
        src, p_src = layouts.place_operand(spec, lay, "src", [pics(p) for p in c["src"]], n, fill)
        best = best_records(dsp.lr_sgr_search_frame(cdef, dblk, src, w, h, bd, us, 0, 16, scratch=scratch_for(dsp, c, n))).reshape(n, -1)[-1]
        assert np.array_equal(best["ep"], full[:, 0]) and np.array_equal(best["xqd"], full[:, 1:3]) and np.array_equal(best["sse"], full[:, 3]), ("search", n)
        layouts.assert_all_intact(p_cdef + p_dblk + p_src, fill)


def test_stack_of_two_pictures_captured_into_a_graph(dsp):
    """statistics, walk and search on a stack of two pictures of one geometry, captured once and replayed twice with the outputs and the
    scratch overwritten in between: the same bytes each time; picture 0 equals the fixture, picture 1 (the picture turned round) the
    same calls on it alone"""
    c = sc.case("u64")
    w, h, bd, us = geometry(c)
    turn = lambda p: np.ascontiguousarray(p[::-1, ::-1])
    stack = lambda key: tuple(torch.stack([dev(p), dev(turn(p))]) for p in c[key])
    cdef, dblk, src = stack("cdef"), stack("dblk"), stack("src")
    one = lambda planes: tuple(p[1].contiguous() for p in planes)
    lo, hi = 2, 15
    alone = dsp.lr_sgr_search_frame(one(cdef), one(dblk), one(src), w, h, bd, us, lo, hi)
    n = c["offsets"][3]
    stats = torch.zeros((2, n, 16, 5), dtype=torch.int64, device="cuda")
    walk = torch.zeros((2, n, 16, 24), dtype=torch.uint8, device="cuda")
    best = torch.zeros((2, n, 24), dtype=torch.uint8, device="cuda")
    s1, s2 = scratch_for(dsp, c, 2, lo, hi), scratch_for(dsp, c, 2, lo, hi)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            dsp.lr_sgr_stats_frame(cdef, src, w, h, bd, us, lo, hi, stats=stats, scratch=s1)
            dsp.lr_sgr_walk_frame(cdef, src, w, h, bd, us, s1, lo, hi, stats=stats, walk=walk)
            dsp.lr_sgr_search_frame(cdef, dblk, src, w, h, bd, us, lo, hi, best=best, scratch=s2)
    results = []
    for fill in (7, 9):
        for t in (stats[:, :, lo:hi], walk[:, :, lo:hi], best, s1, s2):
            t.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        results.append([t.cpu().numpy().copy() for t in (stats[:, :, lo:hi], walk[:, :, lo:hi], best)])
    for x, y in zip(*results):
        assert np.array_equal(x, y)
    assert np.array_equal(results[0][0][0], model_sums(c)[:, lo:hi])
    check_walk(c, walk_records(walk)[0], lo, hi, "picture 0 of the stack")
    b = best_records(best)
    ep = lo + np.argmin(c["err"][:, lo:hi], axis=1)
    assert np.array_equal(b[0]["ep"], ep) and np.array_equal(b[0]["xqd"], c["final"][np.arange(n), ep]) and np.array_equal(b[0]["proj_err"], c["err"][np.arange(n), ep])
    assert torch.equal(best[1], alone) and not torch.equal(best[0], best[1])
    w1 = walk_records(walk)[1][:, lo:hi]
    assert np.array_equal(b[1]["proj_err"], w1["err"].min(axis=1)) and not np.array_equal(results[0][0][0], results[0][0][1])


@pytest.mark.parametrize("name", [n for n in CASES if "results" in sc.case(n)])
def test_lr_search_end_to_end_equals_rest_finish_search_on_real_search_results(dsp, name):
    """dsp.lr_search_units (the unfiltered errors, the Wiener search, the self-guided search over the full range) gives the recorded unit
    results; svt_hip_lr_finish on them, under every recorded setting, the reference's frame types and unit records; dsp.lr_search is the
    two in one call; and the picture restored under its decision is the plain model's"""
    c = sc.case(name)
    w, h, bd, us = geometry(c)
    cdef, dblk, src = (tuple(dev(p) for p in c[k]) for k in ("cdef", "dblk", "src"))
    res, cnt = dsp.lr_search_units(cdef, dblk, src, w, h, bd, us, c["wiener_win"])
    want = c["results"]
    for f in ("sse", "ep", "xqd"):
        assert np.array_equal(res[f], want[f]), (name, f, np.argwhere(res[f] != want[f])[:4].tolist())
    usable = want["sse"][:, 1] != np.iinfo(np.int64).max
    assert np.array_equal(res["vfilter"][usable], want["vfilter"][usable]) and np.array_equal(res["hfilter"][usable], want["hfilter"][usable])
    assert np.array_equal(cnt, c["cnt"][0])
    g = sc.fixture()
    for i, (costs, row) in enumerate(zip(g["finishes"], c["fin_types"])):
        for plane in range(3):
            a, b = c["offsets"][plane], c["offsets"][plane + 1]
            ft, un = dsp.lr_finish(plane, int(row[0]), costs, res[a:b], dsp.lib)
            wu = c["fin_units"][i][a:b]
            assert ft == int(row[1 + plane]), (name, i, plane)
            assert [int(v) for v in un["type"]] == [int(v) for v in wu["type"]], (name, i, plane)
            for g_, w_ in zip(un, wu):
                assert (g_["vfilter"].tolist(), g_["hfilter"].tolist()) == (w_["vfilter"].tolist(), w_["hfilter"].tolist()) if int(w_["type"]) == 1 else \
                    (int(g_["ep"]), g_["xqd"].tolist()) == (int(w_["ep"]), w_["xqd"].tolist()), (name, i, plane)
    row = c["fin_types"][0]
    types, units, cnt2 = dsp.lr_search(cdef, dblk, src, w, h, bd, us, c["wiener_win"], int(row[0]), g["finishes"][0])
    assert types == [int(v) for v in row[1:]] and np.array_equal(cnt2, cnt)
    assert units["type"].tolist() == c["fin_units"][0]["type"].tolist()
    out = dsp.lr_apply_frame(cdef, dblk, w, h, bd, us, types, units)
    m = dict(c)
    m["frame_type"], m["units"] = types, units
    check_planes(out, lc.model_apply(m), w, h, None, "the picture under the search's decision")
