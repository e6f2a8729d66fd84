"""GPU: svt_hip_cdef_search_frame / svt_hip_cdef_apply_frame against the reference.  tests/golden/cdef.npz holds, per small picture,
the reference's mse_seg table, block counts and applied pictures (written by tests/golden/make_golden_cdef.py from libsvtref.so's own
cdef_filter_fb / compute_cdef_dist); at scale (one 1920x1080 picture) the chroma half of the table is checked against a torch
restatement of the integer arithmetic written here, the luma half against the live libsvtref.so on a sample of filter blocks (when
oracle/_ref/libsvtref.so is present), and the apply against the search itself.  Every comparison is an equality: the luma distortion's
binary64 expression is reproduced bit for bit or the test fails."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_cdef as mg      # noqa: E402  (the fixture's glue: case list, filter-block loop over the live reference)

sys.path.insert(0, os.path.join(ROOT, "tests"))
import layouts                     # noqa: E402
import poison                      # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "cdef.npz")
CASES = [c[0] for c in mg.CASES]
ERR_INVALID = -2
SENT = 0x5A5A5A5A5A5A5A5A
LARGE = 30000


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


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


def case_of(g, n, pad=0):
    bd, w, h, q = (int(v) for v in g[n + "_meta"])
    rec = tuple(dev(g[n + "_rec_" + c], pad, 201) for c in "yuv")
    src = tuple(dev(g[n + "_src_" + c], pad, 202) for c in "yuv")
    return bd, w, h, q, rec, src, dev(g[n + "_skip"], pad, 0)


def sentinels(nfb, lead=()):
    return (torch.full(lead + (2, nfb, 64), SENT, dtype=torch.int64, device="cuda"),
            torch.full(lead + (nfb,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("window", [(0, 64), (0, 8), (9, 23)])
@pytest.mark.parametrize("name", CASES)
def test_search_equals_the_reference_table(dsp, gold, name, window):
    bd, w, h, q, rec, src, skip = case_of(gold, name, pad=8 if name in "be" else 0)
    want = gold[name + "_mse"].astype(np.int64).copy()
    want[:, :, :window[0]] = 0
    want[:, :, window[1]:] = 0
    mse, count = sentinels(want.shape[1])
    dsp.cdef_search_frame(rec, src, skip, w, h, bd, q, window[0], window[1], mse=mse, count=count)
    torch.cuda.synchronize()
    got = mse.cpu().numpy()
    assert np.array_equal(count.cpu().numpy(), gold[name + "_count"])
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, len(bad), bad[:5], [(int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:5]])


@pytest.mark.parametrize("name", CASES)
def test_apply_equals_the_reference_picture_and_stays_inside_it(dsp, gold, name):
    bd, w, h, q, rec, src, skip = case_of(gold, name, pad=8)
    dst = tuple(torch.full_like(r, 93) for r in rec)
    ys, us = torch.from_numpy(gold[name + "_ystr"]).cuda(), torch.from_numpy(gold[name + "_ustr"]).cuda()
    dsp.cdef_apply_frame(rec, skip, ys, us, w, h, bd, q, dst=dst)
    torch.cuda.synchronize()
    for i, c in enumerate("yuv"):
        want = gold[name + "_out_" + c]
        got = dst[i].cpu().numpy().view(want.dtype)
        ph, pw = want.shape
        assert np.array_equal(got[:ph, :pw], want), (name, c, np.argwhere(got[:ph, :pw] != want)[:5])
        assert (got[ph:] == 93).all() and (got[:, pw:] == 93).all(), (name, c)


def test_stack_under_a_captured_graph_replayed_twice(dsp, gold):
    """cases b and c (one geometry, one base_qindex) as a stack of two pictures, captured once, replayed twice"""
    b, c = case_of(gold, "b"), case_of(gold, "c")
    assert b[:4] == c[:4]
    bd, w, h, q = b[:4]
    rec = tuple(torch.stack([x, y]).contiguous() for x, y in zip(b[4], c[4]))
    src = tuple(torch.stack([x, y]).contiguous() for x, y in zip(b[5], c[5]))
    skip = torch.stack([b[6], c[6]]).contiguous()
    want = np.stack([gold["b_mse"], gold["c_mse"]]).astype(np.int64)
    mse, count = sentinels(want.shape[2], lead=(2,))
    graph = torch.cuda.CUDAGraph()
    s_ = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s_):
        with torch.cuda.graph(graph, stream=s_):
            dsp.cdef_search_frame(rec, src, skip, w, h, bd, q, 0, 64, mse=mse, count=count)
    torch.cuda.synchronize()
    for _ in range(2):
        mse.fill_(SENT)
        count.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(mse.cpu().numpy(), want)
        assert np.array_equal(count.cpu().numpy(), np.stack([gold["b_count"], gold["c_count"]]))


@pytest.mark.parametrize("names", [("b", "c"), ("e",)], ids=["stack_b_c", "e_10bit"])
@pytest.mark.parametrize("fill", poison.FILLS, ids=lambda f: f"fill{f:02X}")
def test_search_and_apply_with_every_operand_laid_out_differently_equal_the_reference(dsp, gold, names, fill):
    """rec / src / skip (search) and rec / dst / skip (apply): a stride per plane and role that no other plane of the call has, the chroma
    strides unrelated to luma's; cases b and c as a stack of two with a pitch per plane and role, case e (10-bit) alone.  Outputs are
    poisoned (both fill bytes: 8-bit samples), guards checked on every operand.  tests/layouts.py asserts the layouts distinct and a
    mix-up of them harmless before anything is uploaded."""
    n = len(names)
    bd, w, h, q = (int(v) for v in gold[names[0] + "_meta"])
    get = (lambda key: np.stack([gold[m + key] for m in names])) if n == 2 else (lambda key: gold[names[0] + key])
    with poison.poisoned(dsp, fill):
        spec = layouts.cdef_spec("svt_hip_cdef_search_frame", w, h, ("rec", "src"), n)
        lay = layouts.distinct_layouts(spec)
        rec, p_rec = layouts.place_operand(spec, lay, "rec", [get("_rec_" + c) for c in "yuv"], n, fill)
        src, p_src = layouts.place_operand(spec, lay, "src", [get("_src_" + c) for c in "yuv"], n, fill)
        skip, p_skip = layouts.place_operand(spec, lay, "skip", [get("_skip")], n, fill)
        mse, count = dsp.cdef_search_frame(rec, src, skip[0], w, h, bd, q)
        torch.cuda.synchronize()
        assert np.array_equal(count.cpu().numpy(), get("_count"))
        got, want = mse.cpu().numpy(), get("_mse").astype(np.int64)
        assert np.array_equal(got, want), (names, np.argwhere(got != want)[:5].tolist())
        layouts.assert_all_intact(p_rec + p_src + p_skip, fill)

        spec = layouts.cdef_spec("svt_hip_cdef_apply_frame", w, h, ("rec", "dst"), n)
        lay = layouts.distinct_layouts(spec)
        rec, p_rec = layouts.place_operand(spec, lay, "rec", [get("_rec_" + c) for c in "yuv"], n, fill)
        dst, p_dst = layouts.place_operand(spec, lay, "dst", [layouts.poison_like(get("_rec_" + c), fill) for c in "yuv"], n, fill)
        skip, p_skip = layouts.place_operand(spec, lay, "skip", [get("_skip")], n, fill)
        ys, us = torch.from_numpy(get("_ystr")).cuda(), torch.from_numpy(get("_ustr")).cuda()
        dsp.cdef_apply_frame(rec, skip[0], ys, us, w, h, bd, q, dst=dst)
        torch.cuda.synchronize()
        for i, c in enumerate("yuv"):
            want = get("_out_" + c)
            got = dst[i].cpu().numpy().view(want.dtype)
            assert np.array_equal(got, want), (names, c, np.argwhere(got != want)[:5].tolist())
        layouts.assert_all_intact(p_rec + p_skip, fill)
        layouts.assert_all_intact(p_dst, fill, written=True)


def test_invalid_arguments_are_refused_before_any_launch(dsp, gold):
    bd, w, h, q, rec, src, skip = case_of(gold, "a")
    mse, count = sentinels(4)
    dst = tuple(torch.full_like(r, 93) for r in rec)
    st = torch.zeros(4, dtype=torch.int8, device="cuda")
    L, P = dsp.lib, dsp._p

    def search(p, g0=0, g1=64, m=mse, c=count):
        return L.svt_hip_cdef_search_frame(ctypes.addressof(p) if p is not None else None, g0, g1, P(m) if m is not None else None,
                                           P(c) if c is not None else None, dsp._stream())

    def apply(p, a=st, b=st):
        return L.svt_hip_cdef_apply_frame(ctypes.addressof(p) if p is not None else None, P(a) if a is not None else None,
                                          P(b) if b is not None else None, dsp._stream())

    def mk(**kw):
        p = dsp.make_cdef_pic(rec, skip, w, h, bd, q, src=src, dst=dst)
        p.width, p.height, p.bit_depth, p.base_qindex = kw.get("w", w), kw.get("h", h), kw.get("bd", bd), kw.get("q", q)
        return p
    assert search(None) == ERR_INVALID and apply(None) == ERR_INVALID
    for kw in (dict(w=100), dict(h=100), dict(w=0), dict(bd=9), dict(bd=12), dict(q=-1), dict(q=256)):
        assert search(mk(**kw)) == ERR_INVALID, kw
        assert apply(mk(**kw)) == ERR_INVALID, kw
    for g0, g1 in ((-1, 64), (0, 65), (5, 5), (9, 3)):
        assert search(mk(), g0, g1) == ERR_INVALID, (g0, g1)
    assert search(mk(), m=None) == ERR_INVALID and search(mk(), c=None) == ERR_INVALID
    assert apply(mk(), a=None) == ERR_INVALID and apply(mk(), b=None) == ERR_INVALID
    for field, i in (("d_rec", 0), ("d_rec", 2), ("d_src", 1), ("d_skip", None)):
        p = mk()
        if i is None:
            p.d_skip = None
        else:
            getattr(p, field)[i] = None
        assert search(p) == ERR_INVALID, field
    p = mk(); p.d_dst[1] = None
    assert apply(p) == ERR_INVALID
    p = mk(); p.d_dst[0] = p.d_rec[0]
    assert apply(p) == ERR_INVALID
    p = mk(); p.rec_stride[0] = w - 8
    assert search(p) == ERR_INVALID and apply(p) == ERR_INVALID
    p = mk(); p.npics = 0
    assert search(p) == ERR_INVALID
    torch.cuda.synchronize()
    assert (mse == SENT).all() and (count == 0x5A5A5A5A).all() and all((d == 93).all() for d in dst)
    assert b"" != L.svt_hip_last_error()
    assert search(mk()) == 0 and apply(mk()) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# at scale: one 1920x1080 picture
# ---------------------------------------------------------------------------------------------------------------------------
W, H, Q = 1920, 1080, 140


def line_maps():
    i, j = np.mgrid[0:8, 0:8]
    return [i + j, i + j // 2, i, 3 + i - j // 2, 7 + i - j, 3 - i // 2 + j, j, i // 2 + j]


def torch_find_dir(luma):
    """direction of every 8x8 block of an 8-bit luma plane [H, W] -> int64 [H / 8, W / 8] (the costs of cdef_find_dir, restated)"""
    h, w = luma.shape
    x = luma.long().reshape(h // 8, 8, w // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64) - 128
    costs = []
    for d, lm in enumerate(line_maps()):
        p = torch.zeros(x.shape[0], 15, dtype=torch.int64, device=x.device)
        p.index_add_(1, torch.from_numpy(lm.ravel()).to(x.device), x)
        p2 = p * p
        if d in (2, 6):
            c = p2[:, :8].sum(1) * 105
        elif d in (0, 4):
            c = p2[:, 7] * 105
            for i in range(7):
                c = c + (p2[:, i] + p2[:, 14 - i]) * (840 // (i + 1))
        else:
            c = p2[:, 3:8].sum(1) * 105
            for k in range(3):
                c = c + (p2[:, k] + p2[:, 10 - k]) * (840 // (2 * k + 2))
        costs.append(c)
    return torch.stack(costs, 1).argmax(1).reshape(h // 8, w // 8)          # argmax: the first of equal maxima, as the strict '>' scan


def torch_chroma_taps(plane, dirs):
    """plane uint8 [h, w] (chroma), dirs int64 [h / 4, w / 4] -> (x, diffs [12, h, w] in cdef_filter_block's order, min, max)"""
    h, w = plane.shape
    pad = torch.full((h + 4, w + 4), LARGE, dtype=torch.int64, device=plane.device)
    pad[2:-2, 2:-2] = plane.long()
    dmap = dirs.repeat_interleave(4, 0).repeat_interleave(4, 1)
    table = torch.tensor(mg.DIRS, dtype=torch.int64, device=plane.device)            # [8, 2, (dy, dx)]
    yy, xx = torch.meshgrid(torch.arange(h, device=plane.device), torch.arange(w, device=plane.device), indexing="ij")
    x = pad[2:-2, 2:-2]
    diffs, mn, mx = [], x.clone(), x.clone()
    for k in range(2):
        for dd in (dmap, (dmap + 2) & 7, (dmap + 6) & 7):
            dy, dx = table[dd, k, 0], table[dd, k, 1]
            for sg in (1, -1):
                p = pad[yy + 2 + sg * dy, xx + 2 + sg * dx]
                diffs.append(p - x)
                mn = torch.minimum(mn, p)
                mx = torch.where(p != LARGE, torch.maximum(mx, p), mx)
    # order: k0 pri +,-; k0 sec (4); k1 pri +,-; k1 sec (4)
    return x, diffs, mn, mx


def torch_chroma_filter(taps, pri, sec, damping):
    x, diffs, mn, mx = taps

    def constrain(d, thr):
        if thr == 0:
            return torch.zeros_like(d)
        shift = max(0, damping - (thr.bit_length() - 1))
        a = d.abs()
        return d.sign() * torch.minimum(a, (thr - (a >> shift)).clamp(min=0))
    ptaps = (3, 3) if pri & 1 else (4, 2)
    total = torch.zeros_like(x)
    for k in range(2):
        base = 6 * k
        total = total + ptaps[k] * (constrain(diffs[base], pri) + constrain(diffs[base + 1], pri))
        for q in range(2, 6):
            total = total + (2, 1)[k] * constrain(diffs[base + q], sec)
    y = x + ((8 + total - (total < 0).long()) >> 4)
    return torch.maximum(torch.minimum(y, mx), mn)


def per_fb_sum(v, fbsize):
    """[h, w] -> [nvfb * nhfb] sums over fbsize x fbsize tiles (zero padded)"""
    h, w = v.shape
    nv, nh = -(-h // fbsize), -(-w // fbsize)
    p = torch.zeros(nv * fbsize, nh * fbsize, dtype=v.dtype, device=v.device)
    p[:h, :w] = v
    return p.reshape(nv, fbsize, nh, fbsize).sum((1, 3)).reshape(-1)


@pytest.fixture(scope="module")
def scene(dsp):
    rng = np.random.default_rng(1080)
    src, rec = [], []
    for pli in range(3):
        s = mg.smooth_picture(rng, H >> (pli > 0), W >> (pli > 0))
        r = (s + rng.integers(-6, 7, s.shape) + (rng.random(s.shape) < 0.02) * rng.integers(-50, 51, s.shape)).clip(0, 255)
        src.append(s.astype(np.uint8))
        rec.append(r.astype(np.uint8))
    skip = (rng.random((H // 8, W // 8)) < 0.3).astype(np.uint8)
    skip[8:16, 16:24] = 1                                                      # one filter block skipped whole
    d = dict(src=src, rec=rec, skip=skip, dsrc=tuple(dev(p) for p in src), drec=tuple(dev(p) for p in rec), dskip=dev(skip))
    nfb = ((W + 63) // 64) * ((H + 63) // 64)
    mse, count = sentinels(nfb)
    dsp.cdef_search_frame(d["drec"], d["dsrc"], d["dskip"], W, H, 8, Q, 0, 64, mse=mse, count=count)
    torch.cuda.synchronize()
    d["mse"], d["count"] = mse, count
    return d


def test_scale_counts_and_coverage(scene):
    skip = torch.from_numpy(scene["skip"]).cuda()
    want = per_fb_sum((skip == 0).int(), 8)
    assert torch.equal(scene["count"], want.int())
    assert not (scene["mse"] == SENT).any()
    assert (scene["mse"][:, scene["count"] == 0] == 0).all() and (scene["count"] == 0).any()


def test_scale_chroma_equals_the_torch_restatement(scene):
    dirs = torch_find_dir(scene["drec"][0])
    listed = (scene["dskip"] == 0).repeat_interleave(4, 0).repeat_interleave(4, 1)
    taps = [(torch_chroma_taps(scene["drec"][p], dirs), torch_chroma_taps(scene["drec"][p], torch.zeros_like(dirs))) for p in (1, 2)]
    damping = 3 + (Q >> 6) - 1
    for gi in range(64):
        pri, sec = gi // 4, gi % 4 + (gi % 4 == 3)
        want = 0
        for p in (1, 2):
            y = torch_chroma_filter(taps[p - 1][0 if pri else 1], pri, sec, damping)
            e = (y - scene["dsrc"][p].long()) * listed
            want = want + per_fb_sum(e * e, 32)
        got = scene["mse"][1, :, gi]
        assert torch.equal(got, want), (gi, torch.nonzero(got != want)[:5].tolist())


def test_scale_luma_equals_the_live_reference_on_a_sample(scene):
    L = mg.ref_lib()
    if L is None:
        pytest.skip("oracle/_ref/libsvtref.so is not built here: the 1080p luma table is not compared with the live reference "
                    "(the fixture cases still pin luma to it)")
    nhfb, nvfb = (W + 63) // 64, (H + 63) // 64
    src16 = [np.ascontiguousarray(p.astype(np.uint16)) for p in scene["src"]]
    got = scene["mse"].cpu().numpy()
    rng = np.random.default_rng(5)
    sample = {(0, 0), (0, nhfb - 1), (nvfb - 1, 0), (nvfb - 1, nhfb - 1), (nvfb - 1, nhfb // 2), (nvfb // 2, nhfb - 1)}
    sample |= {(int(rng.integers(nvfb)), int(rng.integers(nhfb))) for _ in range(10)}
    for fbr, fbc in sorted(sample):
        r = mg.ref_search_fb(L, scene["rec"], src16, scene["skip"], fbr, fbc, 8, Q)
        fb = fbr * nhfb + fbc
        want = np.zeros((2, 64), np.int64) if r is None else r[0].astype(np.int64)
        assert np.array_equal(got[:, fb], want), (fbr, fbc, np.argwhere(got[:, fb] != want)[:5])


def test_scale_apply_agrees_with_the_search(dsp, scene):
    """apply with each filter block's argmin strengths; the search's own chroma entry at that strength is the squared error between the
    applied chroma planes and the source over the listed blocks, and so is luma's plain squared error whenever the picked strength is 0"""
    mse, count = scene["mse"], scene["count"]
    ys = mse[0].argmin(1).to(torch.int8)
    us = mse[1].argmin(1).to(torch.int8)
    ys[count == 0] = -1
    us[count == 0] = -1
    dst = tuple(torch.full_like(r, 93) for r in scene["drec"])
    dsp.cdef_apply_frame(scene["drec"], scene["dskip"], ys, us, W, H, 8, Q, dst=dst)
    torch.cuda.synchronize()
    listed = (scene["dskip"] == 0).repeat_interleave(4, 0).repeat_interleave(4, 1)
    sse = 0
    for p in (1, 2):
        e = (dst[p].long() - scene["dsrc"][p].long()) * listed
        sse = sse + per_fb_sum(e * e, 32)
    pick = us.long().clamp(min=0)
    want = mse[1].gather(1, pick[:, None])[:, 0]
    assert torch.equal(sse, want), torch.nonzero(sse != want)[:5].tolist()
    # skipped blocks and left-out filter blocks are copies of the input, in all planes
    keep = ~(scene["dskip"] == 0)
    assert torch.equal(dst[0][keep.repeat_interleave(8, 0).repeat_interleave(8, 1)], scene["drec"][0][keep.repeat_interleave(8, 0).repeat_interleave(8, 1)])
    for p in (1, 2):
        assert torch.equal(dst[p][~listed], scene["drec"][p][~listed])
    assert (dst[0] != scene["drec"][0]).any() and (dst[1] != scene["drec"][1]).any()
