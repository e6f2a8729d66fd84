"""GPU: the back half of the encoder chained on the device on ONE real picture, stage by stage against the reference
(tests/golden/back_end.npz, written by tests/golden/make_golden_back_end.py from the reference's own functions on the 352 x 224 window
of tests/golden/real_picture.npz; the inputs are the stated functions of tests/back_end_cases.py).  This module is the executable
statement of the back end's data flow:

  1  svt_hip_partition_decide_frame     leaves, costs                                   -> d_sq, d_final, d_final_count
  2  svt_hip_recon_final_frame          d_final / d_final_count of 1, records, groups   -> planes (inter blocks), status, stream offsets
  3  svt_hip_intra_encode_frame         the same list, the planes of 2 (in place)       -> planes (intra blocks), status, result, stream
  4  svt_hip_dlf_mi_frame               the same list, svt_hip_dlf_info from 3's eobs   -> the mode-info grid
  5  svt_hip_dlf_search_frame           the planes of 3, the source, the grid of 4      -> ss_err[plane][level]; svt_hip_dlf_pick_level
  6  svt_hip_dlf_apply_frame            the planes of 3, the grid of 4, the levels of 5 -> the deblocked planes
  7  svt_hip_cdef_search_frame / _apply the planes of 6, the skip map of 4's grid       -> the table, the filtered planes

Every stage reads the device tensors the stage before it wrote.  The contract between the calls:
  src      one numbering for d_cost, svt_hip_md_decision, svt_hip_intra_enc_blk and svt_hip_dlf_info: the leaves of one block size are
           numbered contiguously, sizes ascending (back_end_cases.leaf_lists), so that a source group of call 2 is one block size and
           the list call 1 writes is handed to calls 2, 3 and 4 as it is - no renumbered copy exists.
  groups   d_best_pred of every group is gathered on the device, with torch indexing, from the uploaded reference planes (an inter
           block's prediction is the co-located block of the reference picture; its record has eob 0, so call 2 copies it).  Call 2
           reconstructs EVERY entry - the stream offsets of 2 and 3 are then equal, as include/svt_hip_dsp.h promises - and an intra
           entry's "prediction" is the fill byte: before call 3 the planes hold the fill wherever no inter block lies, under both fill
           bytes, so a predictor that read a sample of a block not yet coded would differ between the two scenes.
  info     ref_frame0 0 / 1, mode the luma mode (GLOBALMV / NEWMV for inter), skip by update_av1_mi_map's rule from call 3's eobs
           (an inter entry: eob 0), formed with torch operations, no eob crosses to the host.
Taken off the device path: the walk of the level pick (svt_hip_dlf_pick_level, host) and the CDEF argmin (numpy, first of equal
minima).  Every output is allocated poisoned (tests/poison.py; the scene runs once per fill byte), every comparison is an equality over
all entries, and what a call may not write must still hold the fill."""
import os
import sys

import numpy as np
import pytest
import torch

import poison
import svtlibs
import back_end_cases as bc
from back_end_cases import mg, mi, mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_real_picture as mg_real      # noqa: E402

W, H, NSB, MAX_FINAL = bc.W, bc.H, bc.NSB, bc.MAX_FINAL
MI_SPARE = (2, 3)                                 # rows / columns of grid beyond the picture's, which no call may write


@pytest.fixture(scope="module")
def gold():
    g = bc.load()
    geom, rgeom = bc.geometry()
    pics = dict(src=[g[f"src{p}"] for p in range(3)], ref=[g[f"ref{p}"] for p in range(3)])
    case, groups = bc.partition_case(pics, geom)
    final = bc.padded_final(g["part_final"], g["part_count"])
    tabs = bc.src_tables(final, g["part_count"], pics, geom, rgeom, len(case["leaf"]))
    for v in g.values():
        v.setflags(write=False)
    return dict(g=g, geom=geom, rgeom=rgeom, pics=pics, case=case, groups=groups, final=final, tabs=tabs)


def up(a):
    a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a)        # (the fixture's arrays are read-only: upload a copy)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def records(a):
    return up(a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)))


class Scene:
    """the stages of the chain, each run at most once (on first use) inside a poisoned block of its own; need(name) holds what it wrote"""

    def __init__(self, dsp, gold, fill):
        self.dsp, self.gold, self.g, self.fill, self.done = dsp, gold, gold["g"], fill, {}
        g, case, tabs = self.g, gold["case"], gold["tabs"]
        self.nsrc = len(case["leaf"])
        assert self.nsrc == int(g["nsrc"])
        self.q = int(g["qindex"])
        self.qrow = {k: v[self.q].copy() for k, v in svtlibs.quant_tables(8).items()}
        self.sharp = int(g["dlf_sharp"])
        # uploaded once
        self.part_in = dict(sb=records(case["sb"]), leaf=records(case["leaf"]), cost=up(case["cost"]), partition_bits=up(case["bits"]))
        self.src = [up(p) for p in bc.in_planes(gold["pics"]["src"])]
        self.ref = [up(p) for p in gold["pics"]["ref"]]
        self.blk = records(tabs["blk"])
        self.decision = records(tabs["decision"])
        self.inter_mode = up(tabs["inter_mode"])
        self.has_uv = up(gold["geom"]["has_uv"])
        self.tables = torch.from_numpy(dsp.intra_encode_tables()).cuda()
        live = np.argwhere(np.arange(MAX_FINAL)[None] < g["part_count"][:, None])
        self.live_sb, self.live_k = up(live[:, 0]), up(live[:, 1])            # where the live entries are (not what they hold)
        self.groups = self.gather_groups()

    def need(self, name):
        if name not in self.done:
            with poison.poisoned(self.dsp, self.fill):
                self.done[name] = getattr(self, "run_" + name)()
                torch.cuda.synchronize()
            for key in ("buffers", "second", "warm"):                                # the buffers outlive the block they were allocated in
                if isinstance(self.done.get(key), dict):
                    self.check_guards(self.done[key])
        return self.done[name]

    def check_guards(self, b):
        """the guards of buffers that outlive the block they were allocated in"""
        for k, v in b.items():
            for t in (v if isinstance(v, list) else [v]) if not k.startswith("scratch") else ():
                poison.assert_guards(t, self.fill, k)

    # -- the source groups of call 2 ----------------------------------------------------------------------------------------------
    def gather_groups(self):
        """per block size the dense predictions of its records, gathered on the device from the reference planes; an intra record's
        are the fill byte"""
        gold = self.gold
        x, y, _ = bc.leaf_positions(gold["geom"], gold["case"]["sb"], gold["case"]["leaf"])
        intra = self.blk[:, 0] != 0
        out = []
        for first, n, b in gold["groups"]:
            xs, ys = up(x[first:first + n]), up(y[first:first + n])
            w, h = mr.BS_W[b], mr.BS_H[b]
            cw, ch = max(w // 2, 4), max(h // 2, 4)
            pred, dq = [], []
            for p in range(3):
                px, py, pw, ph = (xs, ys, w, h) if p == 0 else (((xs >> 3) << 3) >> 1, ((ys >> 3) << 3) >> 1, cw, ch)
                rows = py[:, None, None] + torch.arange(ph, device="cuda")[None, :, None]
                cols = px[:, None, None] + torch.arange(pw, device="cuda")[None, None, :]
                t = self.ref[p][rows, cols]
                pred.append(torch.where(intra[first:first + n, None, None], torch.full_like(t, self.fill), t).contiguous())
                dq.append(torch.zeros((n, min(pw, 32) * min(ph, 32)), dtype=torch.int32, device="cuda"))
            out.append(dict(src_first=first, nblocks=n, bsize=b, tx_type_uv=0, best_pred=pred, best_dqcoeff=dq))
        return out

    # -- 1 ------------------------------------------------------------------------------------------------------------------------
    def run_partition(self):
        dev, case = self.dsp.device, self.gold["case"]
        a = dict(self.part_in, pic_width=W, pic_height=H, slice_is_intra=int(case["slice_is_intra"]),
                 sq=poison.tensor((NSB, mg.NSQ, 16), torch.uint8, dev), final_count=poison.tensor((NSB,), torch.int32, dev),
                 final=poison.tensor((NSB, MAX_FINAL, 12), torch.uint8, dev))
        a["lambda"] = int(case["lam"])
        assert self.dsp.partition_decide_frame(a) == 0, self.dsp.lib.svt_hip_last_error()
        return a

    # -- 2 .. 7: every stage takes what it reads, and `out`, the buffers of an earlier run to write again ---------------------------
    def buffers(self):
        """fresh poisoned outputs (and scratch) of stages 2 .. 7"""
        dsp, dev = self.dsp, self.dsp.device
        planes = lambda: [poison.tensor((bc.ROWS >> (p > 0), bc.STRIDE >> (p > 0)), torch.uint8, dev) for p in range(3)]
        return dict(
            recon=planes(), status2=poison.tensor((NSB, MAX_FINAL), torch.uint8, dev), offset2=poison.tensor((NSB, MAX_FINAL, 2), torch.int32, dev),
            scratch2=torch.empty((dsp.recon_final_scratch_bytes(NSB),), dtype=torch.uint8, device=dev),
            status3=poison.tensor((1, NSB, MAX_FINAL), torch.uint8, dev), result=poison.tensor((1, NSB, MAX_FINAL, 8), torch.uint8, dev),
            offset3=poison.tensor((1, NSB, MAX_FINAL, 2), torch.int32, dev), sbq=[poison.tensor((1, NSB, mi.SPAN[p]), torch.int32, dev) for p in range(3)],
            scratch3=torch.empty((dsp.intra_encode_scratch_bytes(1, NSB),), dtype=torch.uint8, device=dev),
            info=poison.tensor((self.nsrc, 4), torch.uint8, dev), mi=poison.tensor((H // 4 + MI_SPARE[0], W // 4 + MI_SPARE[1], 4), torch.uint8, dev),
            sse=poison.tensor((3, 64), torch.int64, dev), scratch5=torch.empty((dsp.dlf_search_scratch_bytes(W, H, 1),), dtype=torch.uint8, device=dev),
            dlf=planes(), dlf_in_place=planes(), dlf_delta=planes(),
            mse=poison.tensor((2, NSB, 64), torch.int64, dev), count=poison.tensor((NSB,), torch.int32, dev), cdef=planes())

    def outputs(self, b):
        for k, v in b.items():
            if not k.startswith("scratch"):
                yield from (v if isinstance(v, list) else [v])

    def recon_final(self, part, b):
        a = dict(final=part["final"], final_count=part["final_count"], decision=self.decision, groups=self.groups, planes=3, recon=b["recon"],
                 width=list(bc.PW), height=list(bc.PH), status=b["status2"], coeff_offset=b["offset2"], scratch=b["scratch2"])
        assert self.dsp.recon_final_frame(a) == 0, self.dsp.lib.svt_hip_last_error()

    def intra(self, part, b):
        a = dict(npics=1, sb_cols=bc.SB_COLS, sb_rows=bc.SB_ROWS, final=part["final"], final_count=part["final_count"], blk=self.blk, src=self.src,
                 recon=b["recon"], width=list(bc.PW), height=list(bc.PH), q_luma=self.qrow, q_chroma=self.qrow, tables=self.tables,
                 status=b["status3"], result=b["result"], coeff_offset=b["offset3"], sb_qcoeff=b["sbq"], scratch=b["scratch3"])
        assert self.dsp.intra_encode_frame(a) == 0, self.dsp.lib.svt_hip_last_error()

    def grid(self, part, b):
        """svt_hip_dlf_info per src with torch operations from the device's list, the device's eobs and the blk table; then call 4"""
        entry = part["final"][self.live_sb, self.live_k]                      # uint8 [n, 12] of the live entries
        mds = (entry[:, 0:2].contiguous().view(torch.int16).long() & 0xFFFF).squeeze(1)
        src = entry[:, 8:12].contiguous().view(torch.int32).long().squeeze(1)
        blk = self.blk[src]
        intra = blk[:, 0] != 0
        eob = b["result"][0][self.live_sb, self.live_k][:, 0:6].contiguous().view(torch.int16)
        eob = torch.where(intra[:, None], eob, torch.zeros_like(eob))         # an inter entry is a skip block: the intra pass wrote no row
        has_uv = self.has_uv[mds] != 0
        skip = (eob[:, 0] == 0) & (~has_uv | ((eob[:, 1] == 0) & (eob[:, 2] == 0)))
        mode = torch.where(intra, blk[:, 1], self.inter_mode[src])
        rows = torch.stack([(~intra).to(torch.uint8), mode, skip.to(torch.uint8), torch.zeros_like(mode)], 1)
        b["info"].zero_()
        b["info"][src] = rows
        self.dsp.dlf_mi_frame(part["final"], part["final_count"], b["info"], b["mi"], mi_cols=W // 4, mi_rows=H // 4)

    def search(self, b, masks=(-1, -1, -1), sse=None):
        return self.dsp.dlf_search_frame(tuple(b["recon"]), tuple(self.src), b["mi"], W, H, 8, masks=masks, sharpness=self.sharp,
                                         sse=b["sse"] if sse is None else sse, scratch=b["scratch5"])

    def apply(self, b, levels):
        lv = [int(v) for v in levels]
        self.dsp.dlf_apply_frame(tuple(b["recon"]), b["mi"], W, H, 8, lv, sharpness=self.sharp, dst=tuple(b["dlf"]))
        for dst, src in zip(b["dlf_in_place"], b["recon"]):
            dst.copy_(src)
        self.dsp.dlf_apply_frame(tuple(b["dlf_in_place"]), b["mi"], W, H, 8, lv, sharpness=self.sharp, in_place=True)
        rd, md = bc.delta_of(lv)
        self.dsp.dlf_apply_frame(tuple(b["recon"]), b["mi"], W, H, 8, lv, sharpness=self.sharp, ref_deltas=rd, mode_deltas=md, dst=tuple(b["dlf_delta"]))

    def skip_map(self, b):
        """the CDEF skip map from the DEVICE's grid, with torch operations"""
        s = b["mi"][:H // 4, :W // 4, 2] >> 7                               # all four units of an 8x8 (is_8x8_block_skip)
        return (s[::2, ::2] & s[::2, 1::2] & s[1::2, ::2] & s[1::2, 1::2]).contiguous()

    def cdef_search(self, b):
        self.dsp.cdef_search_frame(tuple(b["dlf"]), tuple(self.src), self.skip_map(b), W, H, 8, self.q, mse=b["mse"], count=b["count"])

    def cdef_apply(self, b, strengths):
        self.dsp.cdef_apply_frame(tuple(b["dlf"]), self.skip_map(b), strengths[0], strengths[1], W, H, 8, self.q, dst=tuple(b["cdef"]))

    def chain(self, b, levels, strengths):
        """stages 2 .. 7 into the buffers b, nothing in between waits for the host: the levels and the strengths are given"""
        part = self.need("partition")
        self.recon_final(part, b)
        self.intra(part, b)
        self.grid(part, b)
        self.search(b)
        self.apply(b, levels)
        self.cdef_search(b)
        self.cdef_apply(b, strengths)

    # the stage-by-stage run: one set of buffers, each stage on first use
    def run_buffers(self):
        return self.buffers()

    def run_recon_final(self):
        b = self.need("buffers")
        self.recon_final(self.need("partition"), b)
        torch.cuda.synchronize()
        return dict(planes=[t.clone() for t in b["recon"]])                 # call 3 works in place: what call 2 left, kept for the tests

    def run_intra(self):
        self.need("recon_final")
        self.intra(self.need("partition"), self.need("buffers"))

    def run_grid(self):
        self.need("intra")
        self.grid(self.need("partition"), self.need("buffers"))

    def run_search(self):
        self.need("grid")
        self.search(self.need("buffers"))

    def picked_levels(self):
        """svt_hip_dlf_pick_level over the DEVICE's table from both start rows -> [[l, l, u, v]] (luma walks from the previous
        filter_level_u, Cb from u, Cr from v)"""
        self.need("search")
        table = self.need("buffers")["sse"].cpu().numpy()
        out = []
        for last in self.g["dlf_starts"].tolist():
            picks = [self.dsp.dlf_pick_level(table[plane], start, bc.LOOP_FILTER_MODE, bc.ONLY_4X4) for plane, start in ((0, last[2]), (1, last[2]), (2, last[3]))]
            assert all(kind == "level" for kind, _ in picks), picks
            out.append([picks[0][1], picks[0][1], picks[1][1], picks[2][1]])
        return out

    def run_apply(self):
        self.apply(self.need("buffers"), self.picked_levels()[0])

    def run_cdef_search(self):
        self.need("apply")
        self.cdef_search(self.need("buffers"))

    def strengths(self):
        """the argmin strengths of the device's own table, decided on the host (numpy's argmin: the first of equal minima)"""
        self.need("cdef_search")
        b = self.need("buffers")
        ys, us = mg_real.argmin_strengths(b["mse"].cpu().numpy().view(np.uint64), b["count"].cpu().numpy())
        return up(ys), up(us)

    def run_cdef_apply(self):
        self.cdef_apply(self.need("buffers"), self.strengths())

    def decisions(self):
        """the levels and the strengths of the first run: what a run that never waits for the host is given"""
        if "decisions" not in self.done:
            self.need("cdef_apply")
            self.done["decisions"] = (self.picked_levels()[0], self.strengths())
        return self.done["decisions"]

    def run_second(self):
        """the chain once more into fresh poisoned outputs"""
        levels, strengths = self.decisions()
        b = self.buffers()
        self.chain(b, levels, strengths)
        return b

    run_warm = run_second                                                   # and a third time: the warm run of the graph's buffers


@pytest.fixture(scope="module", params=poison.FILLS, ids=[f"fill{f:02X}" for f in poison.FILLS])
def scene(request, dsp, gold):
    return Scene(dsp, gold, request.param)


def fill32(scene):
    return np.frombuffer(bytes([scene.fill] * 4), np.int32)[0]


def live_of(g):
    return np.arange(MAX_FINAL)[None] < g["part_count"][:, None]


def assert_picture(scene, planes, want, what, mask=None, rest=None):
    """planes [ROWS, STRIDE] against the W x H pictures `want` where `mask` is set (everywhere without one); elsewhere `rest` (the fill
    without one), and the fill outside the picture"""
    for p, t in enumerate(planes):
        got = t.cpu().numpy()
        pic = got[:bc.PH[p], :bc.PW[p]]
        m = np.ones(pic.shape, bool) if mask is None else mask[p]
        bad = np.argwhere((pic != want[p]) & m)
        assert not len(bad), (what, p, len(bad), bad[:4].tolist())
        other = np.full(pic.shape, scene.fill, np.uint8) if rest is None else rest[p][:bc.PH[p], :bc.PW[p]]
        assert np.array_equal(pic[~m], other[~m]), (what, p, "a sample outside the mask changed")
        assert (got[bc.PH[p]:] == scene.fill).all() and (got[:, bc.PW[p]:] == scene.fill).all(), (what, p, "a sample outside the picture was written")


def test_1_partition_decision_gives_the_references_squares_and_final_list(scene, gold):
    g, a = gold["g"], scene.need("partition")
    got_sq = a["sq"].cpu().numpy().view(mg.SQ_DTYPE).reshape(NSB, mg.NSQ)
    bad = np.argwhere(got_sq != g["part_sq"])
    assert not len(bad), bad[:8].tolist()
    count = a["final_count"].cpu().numpy().view(np.uint32)
    assert np.array_equal(count, g["part_count"])
    got = a["final"].cpu().numpy()
    live = live_of(g)
    assert np.array_equal(got[live].copy().view(bc.FINAL_DTYPE).reshape(-1), g["part_final"])
    assert (got[~live] == scene.fill).all()


def test_2_recon_final_on_the_device_list_copies_the_inter_predictions(scene, gold):
    g = gold["g"]
    snap, b, live = scene.need("recon_final"), scene.need("buffers"), live_of(g)
    assert_picture(scene, snap["planes"], [g[f"ref{p}"] for p in range(3)], "recon_final", mask=[g[f"imask{p}"] for p in range(3)])
    status = b["status2"].cpu().numpy()
    assert (status[live] == 0).all() and (status[~live] == scene.fill).all()
    off = b["offset2"].cpu().numpy()
    assert np.array_equal(off[live].view(np.uint32), g["offset"][live]) and (off[~live] == fill32(scene)).all()


def test_3_intra_encode_on_the_same_list_and_planes_equals_the_reference(scene, gold):
    g = gold["g"]
    scene.need("intra")
    snap, b, live = scene.need("recon_final"), scene.need("buffers"), live_of(g)
    assert_picture(scene, b["recon"], [g[f"rec{p}"] for p in range(3)], "intra", mask=[g[f"rmask{p}"] for p in range(3)],
                   rest=[t.cpu().numpy() for t in snap["planes"]])
    assert_picture(scene, b["recon"], [g[f"rec{p}"] for p in range(3)], "the whole reconstruction")
    status = b["status3"].cpu().numpy()[0]
    assert np.array_equal(status[live], g["status"][live]) and (status[~live] == scene.fill).all()
    assert set(status[live].tolist()) == {mi.OK, mi.R_NOT_INTRA}
    res = b["result"].cpu().numpy()[0]
    want = g["result"].view(np.uint8).reshape(res.shape)
    bad = np.argwhere((res != want).any(-1) & g["resmask"])
    assert not len(bad), (bad[:8].tolist(), res[g["resmask"]][:4], want[g["resmask"]][:4])
    assert (res[~g["resmask"]] == scene.fill).all()
    assert torch.equal(b["offset3"][0], b["offset2"]), "the stream offsets of the intra pass are svt_hip_recon_final_frame's"
    assert np.array_equal(b["offset3"].cpu().numpy()[0][live].view(np.uint32), g["offset"][live])
    for p in range(3):
        got, mask = b["sbq"][p].cpu().numpy()[0], g[f"qmask{p}"]
        bad = np.argwhere((got != g[f"sbq{p}"]) & mask)
        assert not len(bad), (p, bad[:8].tolist())
        assert (got[~mask] == fill32(scene)).all(), p


def test_4_mode_info_from_the_devices_eobs_and_the_grid_scattered_from_the_device_list(scene, gold):
    g = gold["g"]
    scene.need("grid")
    b = scene.need("buffers")
    info = b["info"].cpu().numpy().view(bc.INFO_DTYPE).reshape(-1)
    bad = np.argwhere(info != g["info"])
    assert not len(bad), (bad[:8].tolist(), info[bad[:4, 0]], g["info"][bad[:4, 0]])
    grid = b["mi"].cpu().numpy()
    bad = np.argwhere((grid[:H // 4, :W // 4] != g["mi"]).any(-1))
    assert not len(bad), (bad[:8].tolist(), grid[tuple(bad[0])], g["mi"][tuple(bad[0])])
    assert (grid[H // 4:] == scene.fill).all() and (grid[:, W // 4:] == scene.fill).all()


def test_5_level_search_table_and_the_walk_over_it_pick_the_references_levels(scene, gold):
    g = gold["g"]
    scene.need("search")
    b = scene.need("buffers")
    table = b["sse"].cpu().numpy()
    assert np.array_equal(table.view(np.uint64), g["dlf_table"]), np.argwhere(table.view(np.uint64) != g["dlf_table"])[:8].tolist()
    assert scene.picked_levels() == g["dlf_levels"].tolist()
    assert_picture(scene, b["recon"], [g[f"rec{p}"] for p in range(3)], "the reconstruction after the search")
    # in rounds: an empty table, then only what SVT_HIP_DLF_NEED_LEVEL names
    for last, want in zip(g["dlf_starts"].tolist(), g["dlf_levels"].tolist()):
        for plane, start, level in ((0, last[2], want[0]), (1, last[2], want[2]), (2, last[3], want[3])):
            lazy, asked = np.full(64, -1, np.int64), []
            while True:
                kind, l = scene.dsp.dlf_pick_level(lazy, start, bc.LOOP_FILTER_MODE, bc.ONLY_4X4)
                if kind == "level":
                    break
                assert lazy[l] < 0 and l not in asked and len(asked) < 64
                asked.append(l)
                with poison.poisoned(scene.dsp, scene.fill):
                    one = poison.tensor((3, 64), torch.int64, scene.dsp.device)
                    scene.search(b, masks=tuple((1 << l) if pl == plane else 0 for pl in range(3)), sse=one)
                    torch.cuda.synchronize()
                    one = one.cpu().numpy()
                want_one = np.full((3, 64), -1, np.int64)
                want_one[plane, l] = table[plane, l]
                assert np.array_equal(one, want_one), (plane, l)
                lazy[l] = one[plane, l]
            assert l == level and asked, (plane, start, l, level, asked)


def test_6_deblocking_at_the_picked_levels_equals_the_reference(scene, gold):
    g = gold["g"]
    scene.need("apply")
    b = scene.need("buffers")
    assert_picture(scene, b["dlf"], [g[f"dlf{p}"] for p in range(3)], "into a second buffer")
    assert_picture(scene, b["dlf_in_place"], [g[f"dlf{p}"] for p in range(3)], "in place")
    assert_picture(scene, b["dlf_delta"], [g[f"dlfd{p}"] for p in range(3)], "with ref / mode deltas")
    assert_picture(scene, b["recon"], [g[f"rec{p}"] for p in range(3)], "the input of the two-buffer form")
    assert any(not np.array_equal(g[f"dlf{p}"], g[f"dlfd{p}"]) for p in range(3))


def test_7_cdef_on_the_deblocked_planes_with_the_grids_skip_map_equals_the_reference(scene, gold):
    g = gold["g"]
    scene.need("cdef_search")
    b = scene.need("buffers")
    assert np.array_equal(scene.skip_map(b).cpu().numpy(), bc.skip_map(g["mi"]))
    assert np.array_equal(b["count"].cpu().numpy(), g["cdef_count"])
    mse = b["mse"].cpu().numpy().view(np.uint64)
    assert np.array_equal(mse, g["cdef_mse"]), np.argwhere(mse != g["cdef_mse"])[:8].tolist()
    ys, us = scene.strengths()
    assert np.array_equal(ys.cpu().numpy(), g["cdef_ystr"]) and np.array_equal(us.cpu().numpy(), g["cdef_ustr"])
    scene.need("cdef_apply")
    assert_picture(scene, b["cdef"], [g[f"cdef{p}"] for p in range(3)], "cdef apply")
    assert_picture(scene, b["dlf"], [g[f"dlf{p}"] for p in range(3)], "the input of the cdef apply")


def same_outputs(scene, a, b):
    for (ka, ta), (kb, tb) in zip(((k, t) for k in a if not k.startswith("scratch") for t in (a[k] if isinstance(a[k], list) else [a[k]])),
                                  ((k, t) for k in b if not k.startswith("scratch") for t in (b[k] if isinstance(b[k], list) else [b[k]]))):
        assert ka == kb and torch.equal(ta, tb), ka


def test_8_the_chain_captured_into_a_graph_and_replayed_equals_the_uncaptured_run(scene, gold):
    """stages 2 .. 7 captured once on a side stream after a warm run into the same preallocated outputs and scratch; the apply is
    captured at the picked levels, the CDEF apply at the first run's strengths.  The replay starts from re-poisoned outputs."""
    first, b = scene.need("buffers"), scene.need("warm")
    levels, strengths = scene.decisions()
    assert levels == gold["g"]["dlf_levels"][0].tolist()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            scene.chain(b, levels, strengths)
    torch.cuda.current_stream().wait_stream(side)
    for fill in (scene.fill, scene.fill ^ 0xFF):
        for t in scene.outputs(b):
            t.view(torch.uint8).fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        if fill == scene.fill:
            same_outputs(scene, first, b)
    # under the other fill byte: everything a call writes is the same, what it leaves is that fill
    g = gold["g"]
    was, scene.fill = scene.fill, scene.fill ^ 0xFF
    try:
        assert_picture(scene, b["recon"], [g[f"rec{p}"] for p in range(3)], "replayed reconstruction")
        assert_picture(scene, b["dlf"], [g[f"dlf{p}"] for p in range(3)], "replayed deblocking")
        assert_picture(scene, b["dlf_delta"], [g[f"dlfd{p}"] for p in range(3)], "replayed deblocking with deltas")
        assert_picture(scene, b["cdef"], [g[f"cdef{p}"] for p in range(3)], "replayed cdef")
        assert torch.equal(b["mse"], first["mse"]) and torch.equal(b["sse"], first["sse"]) and torch.equal(b["info"], first["info"])
    finally:
        scene.fill = was


def test_9_the_chain_run_again_into_fresh_outputs_is_byte_equal(scene, gold):
    first, second = scene.need("buffers"), scene.need("second")
    assert first["recon"][0].data_ptr() != second["recon"][0].data_ptr()
    same_outputs(scene, first, second)
