"""GPU: the whole-picture calls on a real picture, chained on the device, against the reference (tests/golden/real_picture.npz, written by
tests/golden/make_golden_real_picture.py from the reference's own functions on a 352 x 224 window of its test clip: smooth gradients
next to hard edges, PUs of one SB that disagree on their vectors, directional intra winners, eob 0 and eob > 10, a dozen CDEF strengths).

One module-scoped scene uploads the three pictures once as raw 4:2:0 frame buffers; each stage then reads the device buffers the stage
before it wrote (svt_hip_picture_import -> _pad -> _decimate -> picture statistics, motion estimation, open-loop intra search, the
encode pass, the CDEF search and the CDEF apply).  Two decisions are taken off the device path: the skip map is formed with torch
operations from the device's eobs, the CDEF strengths are the host's argmin (first of equal minima) of the device's table.  Every
output is allocated poisoned (tests/poison.py; the scene runs once per fill byte, since one fill value can be a true sample) and every
comparison is an equality over all entries."""
import os
import sys

import numpy as np
import pytest
import torch

import poison
import svtlibs
from test_gpu_me_frame import as_arrays as me_arrays
from test_gpu_picture_stats import GOLD_KEY as STATS_GOLD_KEY, KEYS as STATS_KEYS, as_arrays as stats_arrays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_real_picture as mg      # noqa: E402

W, H = mg.W, mg.H
PADS = svtlibs.ME_PADS                       # origin of the full, 1/4 and 1/16 pictures in their buffers; chroma sits at PADS[1] too
SPARE = 5                                    # columns of stride beyond the padded picture, as svtlibs.me_pyramid leaves them
PICS = ("src", "ref0", "ref1")
ME_KEYS = ("best_sad", "best_mv", "area_origin", "bipred_sad", "results")
OIS_SIZES = (8, 16, 32, 64)
CDEF_WINDOWS = ((0, 64), (9, 23))


@pytest.fixture(scope="module")
def gold():
    g = mg.load()
    for v in g.values():
        v.setflags(write=False)
    return g


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def xy_of(blocks):
    return up(np.array([(y << 16) | x for (x, y) in blocks], np.uint32).view(np.int32))


def windowed(table, window):
    want = table.astype(np.int64).copy()
    want[..., :window[0]] = 0
    want[..., window[1]:] = 0
    return want


class Scene:
    """the stages of the chain, each run at most once (on first use) inside a poisoned block of its own; s.<name> holds what it wrote"""

    def __init__(self, dsp, pkg, gold, fill):
        self.dsp, self.pkg, self.g, self.fill = dsp, pkg, gold, fill
        self.done = {}
        self.frames = {p: up(np.concatenate([gold[f"{p}_{n}"].ravel() for n in mg.PLANES if f"{p}_{n}" in gold])) for p in PICS}
        self.qrow = {k: v[int(gold["qindex"])].copy() for k, v in svtlibs.quant_tables(8).items()}
        self.q = int(gold["qindex"])

    def need(self, name):
        if name not in self.done:
            with poison.poisoned(self.dsp, self.fill):
                self.done[name] = getattr(self, "run_" + name)()
                torch.cuda.synchronize()
        return self.done[name]

    def untouched(self, t):
        return bool((t.view(torch.uint8) == self.fill).all())

    # -- input: import -> pad -> decimate ---------------------------------------------------------------------------------
    def run_input(self, out=None):
        """-> {picture: dict(imported=(y, cb, cr), full=, quarter=, sixteenth=)}; `out`: the buffers of an earlier run to write again"""
        d, dsp = out or {}, self.dsp
        for p in PICS:
            chroma = p != "ref1"
            if p not in d:
                y = poison.tensor((H + 2 * PADS[0], W + 2 * PADS[0] + SPARE), torch.uint8, dsp.device)
                c = [poison.tensor((H // 2 + 2 * PADS[1], W // 2 + 2 * PADS[1] + SPARE), torch.uint8, dsp.device) if chroma else None for _ in range(2)]
                d[p] = dict(imported=(y, c[0], c[1]), full=poison.tensor(tuple(y.shape), torch.uint8, dsp.device),
                            quarter=poison.tensor((H // 2 + 2 * PADS[1], W // 2 + 2 * PADS[1] + SPARE), torch.uint8, dsp.device),
                            sixteenth=poison.tensor((H // 4 + 2 * PADS[2], W // 4 + 2 * PADS[2] + SPARE), torch.uint8, dsp.device))
            b = d[p]
            dsp.picture_import(self.frames[p], W, H, b["imported"], PADS[0], PADS[0])
            # the in-place border routine on a buffer that holds only the picture; this buffer feeds every later stage
            o = PADS[0]
            b["full"][o:o + H, o:o + W].copy_(b["imported"][0][o:o + H, o:o + W])
            dsp.picture_pad(b["full"], W, H, o, o)
            dsp.picture_decimate(b["full"][o:, o:], b["full"].stride(0), W, H, b["quarter"], (PADS[1], PADS[1]), b["sixteenth"], (PADS[2], PADS[2]))
        return d

    def luma(self, p):
        """the W x H luma picture inside its padded buffer (a view)"""
        o = PADS[0]
        return self.need("input")[p]["full"][o:o + H, o:o + W]

    def chroma(self, p, i):
        o = PADS[1]
        return self.need("input")[p]["imported"][i][o:o + H // 2, o:o + W // 2]

    # -- picture statistics -----------------------------------------------------------------------------------------------
    def run_stats(self, out=None):
        b = self.need("input")["src"]
        planes = self.dsp.pic_stats_planes([b["full"], b["imported"][1], b["imported"][2], b["sixteenth"]],
                                           [(PADS[0], PADS[0]), (PADS[1], PADS[1]), (PADS[1], PADS[1]), (PADS[2], PADS[2])])
        return {prec: self.dsp.picture_stats_frame(planes, W, H, prec, mg.STATS_REGIONS, out=out[prec] if out else None) for prec in (0, 1)}

    # -- motion estimation ------------------------------------------------------------------------------------------------
    def run_me(self, out=None):
        inp = self.need("input")
        pyr = [self.dsp.me_pyramid([inp[p]["full"], inp[p]["quarter"], inp[p]["sixteenth"]], [(o, o) for o in PADS]) for p in PICS]
        d = {}
        for case in mg.ME_CASES:
            params = self.pkg.MeFrameParams.from_lcu_prm(self.g[f"me_{case}_prm"][0])
            nl = 1 if params.slice_type == 1 else 2
            prev = out[case] if out else None
            d[case] = self.dsp.motion_estimate_frame(pyr[0], pyr[1], pyr[2] if nl == 2 else None, params, 1, out=prev, scratch=prev["_scratch"] if prev else None)
        return d

    # -- open-loop intra search -------------------------------------------------------------------------------------------
    def ois_groups(self):
        """[(bsize, [(sb, md index, x, y)], modes, deltas)] - every block of every size that lies inside the picture"""
        md, raster = mg.ois_blocks()
        out = []
        for bsize in OIS_SIZES:
            rows = [(sb, i, (sb % mg.NSBX) * 64 + x, (sb // mg.NSBX) * 64 + y) for sb in range(mg.NSB) for i, (x, y, s) in enumerate(md)
                    if s == bsize and self.g["ois_valid"][sb, raster(x, y, s)]]
            modes, deltas = self.dsp.ois_candidates(bsize, mg.OIS_TL, mg.OIS_IPM, bool(mg.OIS_ISREF))
            out.append((bsize, rows, modes, deltas))
        return out

    def run_ois(self):
        if "ois_device_groups" not in self.done:              # uploaded once: a graph capture takes no copy from the host
            self.done["ois_device_groups"] = [(xy_of([(x, y) for _, _, x, y in rows]), bsize, modes, deltas) for bsize, rows, modes, deltas in self.ois_groups()]
        groups = self.done["ois_device_groups"]
        return self.dsp.ois_search_frame(self.luma("src"), self.need("input")["src"]["full"].stride(0), W, H, groups)

    def run_ois_general(self):
        """the same call on the general fold path (the non-directional candidates through the per-candidate prediction batches)"""
        assert self.dsp.lib.svt_hip_tune(b"ois_no_nd", 1) == 0
        try:
            return self.run_ois()
        finally:
            self.dsp.lib.svt_hip_tune(b"ois_no_nd", 0)

    # -- encode pass ------------------------------------------------------------------------------------------------------
    def run_encode(self, out=None):
        """source against the list-0 reference co-located, luma 16x16 and chroma 8x8 in one call -> {plane: dict(qcoeff, eob, recon)}"""
        dsp = self.dsp
        d = out or {}
        groups = []
        for i, n in enumerate(mg.PLANES):
            tx = mg.TX_16X16 if i == 0 else mg.TX_8X8
            side = svtlibs.TX_W[tx]
            ph, pw = (H, W) if i == 0 else (H // 2, W // 2)
            src, pred = (self.luma("src"), self.luma("ref0")) if i == 0 else (self.chroma("src", i), self.chroma("ref0", i))
            nblk = (ph // side) * (pw // side)
            if n not in d:
                d[n] = dict(qcoeff=poison.tensor((nblk, side * side), torch.int32, dsp.device), eob=poison.tensor((nblk,), torch.int16, dsp.device),
                            recon=poison.tensor((ph, pw), torch.uint8, dsp.device),
                            xy=xy_of([(x, y) for y in range(0, ph, side) for x in range(0, pw, side)]), iscan=up(svtlibs.scan_tables(tx, mg.DCT_DCT)[1]))
            groups.append(dict(src=src, src_stride=src.stride(0), pred=pred, pred_stride=pred.stride(0), recon=d[n]["recon"], recon_stride=pw,
                               xy=d[n]["xy"], tx_size=tx, tx_type=mg.DCT_DCT, iscan=d[n]["iscan"], qcoeff=d[n]["qcoeff"], eob=d[n]["eob"]))
        arr = dsp.make_frame_groups(groups)
        dsp.encode_recon_frame(arr, self.qrow)
        self.enc_keep = (groups, arr)
        return d

    def device_skip_map(self):
        """the skip map from the DEVICE's eobs, with torch operations on the device"""
        e = self.need("encode")
        z = (e["y"]["eob"] == 0) & (e["cb"]["eob"] == 0) & (e["cr"]["eob"] == 0)
        return z.reshape(H // 16, W // 16).repeat_interleave(2, 0).repeat_interleave(2, 1).to(torch.uint8).contiguous()

    # -- CDEF -------------------------------------------------------------------------------------------------------------
    def cdef_inputs(self, fresh=False):
        """(reconstruction planes the encode pass wrote, dense copies of the source planes, the device's skip map); fresh: copy the
        source planes again (inside a capture: the copy is part of the chain)"""
        e = self.need("encode")
        if fresh or "cdef_src" not in self.done:
            self.done["cdef_src"] = (self.luma("src").contiguous(), self.chroma("src", 1).contiguous(), self.chroma("src", 2).contiguous())
        return tuple(e[n]["recon"] for n in mg.PLANES), self.done["cdef_src"], self.device_skip_map()

    def run_cdef_search(self, out=None):
        rec, src, skip = self.cdef_inputs(fresh=out is not None)
        d = out or {}
        for win in CDEF_WINDOWS:
            if win not in d:
                d[win] = (poison.tensor((2, mg.NSB, 64), torch.int64, self.dsp.device), poison.tensor((mg.NSB,), torch.int32, self.dsp.device))
            self.dsp.cdef_search_frame(rec, src, skip, W, H, 8, self.q, win[0], win[1], mse=d[win][0], count=d[win][1])
        return d

    def device_strengths(self):
        """the argmin strengths of the device's own table, decided on the host (numpy's argmin: the first of equal minima)"""
        mse, count = self.need("cdef_search")[(0, 64)]
        ys, us = mg.argmin_strengths(mse.cpu().numpy().view(np.uint64), count.cpu().numpy())
        return up(ys), up(us)

    def run_cdef_apply(self, out=None, strengths=None):
        """planes 8 samples larger than the picture on every side the call could overrun -> (destination planes, the padded inputs)"""
        rec, _, skip = self.cdef_inputs()
        ys, us = strengths or self.device_strengths()
        big = []
        for t, junk in zip(rec + (skip,), (201, 201, 201, 0)):
            b = torch.full((t.shape[0] + 8, t.shape[1] + 8), junk, dtype=torch.uint8, device=t.device)
            b[:t.shape[0], :t.shape[1]].copy_(t)
            big.append(b)
        dst = out or tuple(poison.tensor(tuple(b.shape), torch.uint8, self.dsp.device) for b in big[:3])
        self.dsp.cdef_apply_frame(tuple(big[:3]), big[3], ys, us, W, H, 8, self.q, dst=dst)
        self.apply_keep = big
        return dst


@pytest.fixture(scope="module", params=poison.FILLS, ids=[f"fill{f:02X}" for f in poison.FILLS])
def scene(request, dsp, pkg, gold):
    return Scene(dsp, pkg, gold, request.param)


def assert_planes(scene, got, want, what):
    """a padded buffer against svtlibs.me_pyramid's plane: the padded picture equal, the spare columns of stride never written"""
    cols = want.shape[1] - SPARE
    a = got.cpu().numpy()
    assert a.shape == want.shape and np.array_equal(a[:, :cols], want[:, :cols]), (what, np.argwhere(a[:, :cols] != want[:, :cols])[:4].tolist())
    assert scene.untouched(got[:, cols:].contiguous()), what


def test_input_import_pad_and_decimate_give_the_references_pyramids(scene, gold):
    d = scene.need("input")
    for p in PICS:
        planes, geo = svtlibs.me_pyramid(gold[f"{p}_y"])
        assert [g[1] for g in geo] == list(PADS)
        assert_planes(scene, d[p]["imported"][0], planes[0], (p, "imported luma"))
        assert_planes(scene, d[p]["full"], planes[0], (p, "padded luma"))
        assert_planes(scene, d[p]["quarter"], planes[1], (p, "quarter"))
        assert_planes(scene, d[p]["sixteenth"], planes[2], (p, "sixteenth"))
        for i, n in ((1, "cb"), (2, "cr")):
            if d[p]["imported"][i] is None:
                assert p == "ref1"
                continue
            want = np.pad(gold[f"{p}_{n}"], PADS[1], mode="edge")
            want = np.concatenate([want, np.zeros((want.shape[0], SPARE), np.uint8)], axis=1)
            assert_planes(scene, d[p]["imported"][i], want, (p, n))


def test_statistics_on_the_device_planes_equal_the_reference(scene, gold):
    res = scene.need("stats")
    for prec in (0, 1):
        got = stats_arrays(res[prec])
        for k in STATS_KEYS:
            gk = STATS_GOLD_KEY.get(k, k)
            want = gold[f"stats_{gk}"] if gk in mg.mg_st.PIC_KEYS else gold[f"stats_p{prec}_{gk}"]
            want = np.asarray(want).reshape(got[k].shape)
            assert got[k].dtype == want.dtype and np.array_equal(got[k], want), (prec, k, np.argwhere(got[k] != want)[:4].tolist())


def assert_me(scene, gold, outs):
    for case, kw in mg.ME_CASES.items():
        nl = 1 if kw["slice_type"] == 1 else 2
        got = me_arrays(scene.dsp, outs[case], nl)
        for k in ("best_sad", "best_mv", "area_origin"):
            want = gold[f"me_{case}_{k}"]
            assert np.array_equal(got[k][:, :nl], want[:, :nl]), (case, k, np.argwhere(got[k][:, :nl] != want[:, :nl])[:4].tolist())
        for k in ("bipred_sad", "results"):
            want = gold[f"me_{case}_{k}"]
            assert np.array_equal(got[k], want), (case, k, np.argwhere(got[k] != want)[:4].tolist())


def test_motion_estimation_on_the_device_pyramids_equals_the_reference_on_every_sb(scene, gold):
    assert_me(scene, gold, scene.need("me"))


def assert_ois(scene, gold, outs):
    checked = 0
    for (bsize, rows, modes, deltas), (dist, best) in zip(scene.ois_groups(), outs):
        n = len(modes)
        sb, i = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        assert (gold["ois_count"][sb, i] == n).all()                    # the host-side candidate list is the reference's
        assert (gold["ois_mode"][sb, i, :n] == modes).all() and (gold["ois_delta"][sb, i, :n] == deltas).all()
        got = dist.cpu().numpy().view(np.uint32)
        want = gold["ois_dist"][sb, i, :n]
        assert np.array_equal(got, want), (bsize, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(best.cpu().numpy(), gold["ois_best"][sb, i]), bsize
        checked += len(rows)
    assert checked == int(gold["ois_valid"].sum())


def test_intra_search_on_the_device_luma_equals_the_reference_on_every_block(scene, gold):
    assert_ois(scene, gold, scene.need("ois"))


def test_intra_search_on_the_general_fold_path_equals_the_reference_on_every_block(scene, gold):
    assert_ois(scene, gold, scene.need("ois_general"))


def assert_encode(gold, enc):
    for n in mg.PLANES:
        q, e, r = (enc[n][k].cpu().numpy() for k in ("qcoeff", "eob", "recon"))
        assert np.array_equal(q, gold[f"enc_{n}_qcoeff"]), (n, np.argwhere(q != gold[f"enc_{n}_qcoeff"])[:4].tolist())
        assert np.array_equal(e.view(np.uint16), gold[f"enc_{n}_eob"]), n
        assert np.array_equal(r, gold[f"enc_{n}_recon"]), (n, np.argwhere(r != gold[f"enc_{n}_recon"])[:4].tolist())


def test_encode_pass_on_the_device_planes_equals_the_reference_and_so_does_the_skip_map(scene, gold):
    assert_encode(gold, scene.need("encode"))
    assert np.array_equal(scene.device_skip_map().cpu().numpy(), gold["skip"])


def assert_cdef_search(gold, tables):
    for win in CDEF_WINDOWS:
        mse, count = tables[win]
        got, want = mse.cpu().numpy(), windowed(gold["cdef_mse"], win)
        assert np.array_equal(count.cpu().numpy(), gold["cdef_count"]), win
        assert np.array_equal(got, want), (win, np.argwhere(got != want)[:4].tolist())


def test_cdef_search_on_the_device_reconstruction_equals_the_references_table(scene, gold):
    assert_cdef_search(gold, scene.need("cdef_search"))


def assert_cdef_apply(scene, gold, dst):
    for i, n in enumerate(mg.PLANES):
        want = gold[f"cdef_out_{n}"]
        got = dst[i].cpu().numpy()
        ph, pw = want.shape
        assert np.array_equal(got[:ph, :pw], want), (n, np.argwhere(got[:ph, :pw] != want)[:4].tolist())
        assert (got[ph:] == scene.fill).all() and (got[:, pw:] == scene.fill).all(), n      # nothing outside the picture


def test_cdef_apply_with_the_devices_own_argmin_strengths_equals_the_references_picture(scene, gold):
    ys, us = scene.device_strengths()
    assert np.array_equal(ys.cpu().numpy(), gold["cdef_ystr"]) and np.array_equal(us.cpu().numpy(), gold["cdef_ustr"])
    assert_cdef_apply(scene, gold, scene.need("cdef_apply"))


# The launch rule of svt_hip_cdef_search_frame: chunks = ceil(TARGET_WAVES / (WAVES_PER_FB_PAIR * filter blocks * pictures)), at most one
# chunk per 8 strengths; a workgroup walks ceil(strengths / chunks) strengths.  With this picture's 24 filter blocks:
#   22 pictures = 528 filter blocks -> ceil(8192 / 4224) = 2 chunks of 32 strengths (21 pictures still give 3 chunks)
#   43 pictures = 1032 filter blocks -> ceil(8192 / 8256) = 1 chunk of all 64 strengths (42 pictures still give 2 chunks)
# A change of the rule's constants moves these counts: the assertions below then say which shape is no longer reached.
CDEF_TARGET_WAVES, CDEF_WAVES_PER_FB_PAIR = 8192, 8


def cdef_chunks(npics, ngi=64):
    wgs = mg.NSB * npics
    return max(1, min(-(-CDEF_TARGET_WAVES // (CDEF_WAVES_PER_FB_PAIR * wgs)), ngi // 8))


@pytest.mark.parametrize("npics,window,chunks", [(22, (0, 64), 2), (43, (0, 64), 1), (43, (3, 61), 1)],
                         ids=["two_chunks_of_32", "one_chunk_of_64", "one_chunk_from_strength_3"])
def test_cdef_search_launch_shapes_on_stacks_of_the_picture(scene, gold, npics, window, chunks):
    assert cdef_chunks(npics, window[1] - window[0]) == chunks and cdef_chunks(npics - 1) == chunks + 1, "the launch rule no longer gives this shape"
    assert mg.NSB * npics == {22: 528, 43: 1032}[npics]
    rec, src, skip = scene.cdef_inputs()
    single = scene.need("cdef_search")[(0, 64)]
    with poison.poisoned(scene.dsp, scene.fill):
        # real copies, one after the other at an explicit pitch (make_cdef_pic passes rows * stride): no picture aliases another
        stack = lambda t: t.unsqueeze(0).repeat(npics, 1, 1).contiguous()
        srec, ssrc, sskip = tuple(stack(t) for t in rec), tuple(stack(t) for t in src), stack(skip)
        assert srec[0].data_ptr() != rec[0].data_ptr() and srec[0].stride(0) == H * W
        mse = poison.tensor((npics, 2, mg.NSB, 64), torch.int64, scene.dsp.device)
        count = poison.tensor((npics, mg.NSB), torch.int32, scene.dsp.device)
        scene.dsp.cdef_search_frame(srec, ssrc, sskip, W, H, 8, scene.q, window[0], window[1], mse=mse, count=count)
        torch.cuda.synchronize()
        want = single[0].clone()
        want[..., :window[0]] = 0
        want[..., window[1]:] = 0
        assert np.array_equal(want.cpu().numpy(), windowed(gold["cdef_mse"], window))
        bad = (mse != want[None]).nonzero()
        assert bad.numel() == 0, bad[:4].tolist()
        assert bool((count == single[1][None]).all())


def test_the_whole_chain_captured_in_a_graph_and_replayed_twice_gives_the_eager_results(scene, gold):
    """every stage into the eager run's own buffers, captured once; the strengths are the eager run's, so nothing inside the capture
    waits for the host.  Each replay starts from re-poisoned outputs."""
    eager = {k: scene.need(k) for k in ("input", "stats", "me", "ois", "encode", "cdef_search", "cdef_apply")}
    strengths = scene.device_strengths()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            scene.run_input(out=eager["input"])
            scene.run_stats(out=eager["stats"])
            scene.run_me(out=eager["me"])
            ois = scene.run_ois()
            scene.run_encode(out=eager["encode"])
            scene.run_cdef_search(out=eager["cdef_search"])
            scene.run_cdef_apply(out=eager["cdef_apply"], strengths=strengths)
    torch.cuda.current_stream().wait_stream(st)

    def outputs():
        for b in eager["input"].values():
            yield from (t for t in b["imported"] if t is not None)
            yield from (b["full"], b["quarter"], b["sixteenth"])
        for res in eager["stats"].values():
            yield from res
        for o in eager["me"].values():
            yield from (o[k] for k in ME_KEYS)
        for dist, best in ois:
            yield from (dist, best)
        for e in eager["encode"].values():
            yield from (e["qcoeff"], e["eob"], e["recon"])
        for mse, count in eager["cdef_search"].values():
            yield from (mse, count)
        yield from eager["cdef_apply"]

    for fill in (scene.fill, scene.fill ^ 0xFF):
        for t in outputs():
            t.view(torch.uint8).fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        was, scene.fill = scene.fill, fill
        try:
            test_input_import_pad_and_decimate_give_the_references_pyramids(scene, gold)
            test_statistics_on_the_device_planes_equal_the_reference(scene, gold)
            assert_me(scene, gold, eager["me"])
            assert_ois(scene, gold, ois)
            assert_encode(gold, eager["encode"])
            assert_cdef_search(gold, eager["cdef_search"])
            assert_cdef_apply(scene, gold, eager["cdef_apply"])
        finally:
            scene.fill = was
