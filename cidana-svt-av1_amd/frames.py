"""Host-side tiling of pictures into the (plane, transform size) groups the frame-level entry point takes
(svt_hip_encode_recon_frame) - BASELINE.json configs[3] (one 1080p yuv420p frame, every CU size) and configs[4] (3840x2160
10-bit, 240 frames, one GOP of 30 frames per rank) - and the fixed-size digest of a pass that ranks all-reduce.

A "pass" over a yuv420p picture at luma size S tiles the luma plane with SxS blocks and both chroma planes with
S/2 x S/2 blocks (S/2 >= 4), DCT_DCT, as SURVEY 8(d) specifies for C4 / C5; partial blocks at the right / bottom edge
are left untouched.  Everything here is plain index arithmetic; the device work is the C ABI's."""
from __future__ import annotations

import numpy as np

from .sharding import DIGEST_MOD

TX_OF_SIDE = {64: 4, 32: 3, 16: 2, 8: 1, 4: 0}          # square TxSize by side
LUMA_SIZES = (64, 32, 16, 8, 4)


def tile_origins(pw: int, ph: int, side: int, side_h: int | None = None):
    """(xy, offsets): block origins x | y << 16 and element offsets y * pw + x of the full side x side (or side x side_h) tiles of a plane"""
    xs = np.arange(0, pw - side + 1, side, dtype=np.uint32)
    ys = np.arange(0, ph - (side_h or side) + 1, side_h or side, dtype=np.uint32)
    xy = ((ys[:, None] << 16) | xs[None, :]).reshape(-1)
    offs = (ys[:, None] * np.uint32(pw) + xs[None, :]).reshape(-1)
    return xy.astype(np.uint32), offs.astype(np.uint32)


class FramePass:
    """Device-side state of every group of one or more passes over one picture: origin tables, scan tables, output
    buffers, and the ctypes group array for svt_hip_encode_recon_frame.  Keeps every tensor alive."""

    def __init__(self, dsp, pkg, planes_src, planes_pred, luma_sizes=LUMA_SIZES, is_16bit=False, keep_coeff=False, tx_types=None, rect_tx_sizes=(),
                 spread_outputs=False):
        """tx_types: {block side: transform type} (default DCT_DCT everywhere); rect_tx_sizes: rectangular TxSize ids (5 .. 18) that
        tile the luma plane too (DCT_DCT), e.g. pkg.TX_SIZE_NAMES.index("TX_16X8")"""
        torch = dsp.torch                     # the module the SvtHipDsp allocates through
        self.dsp, self.torch = dsp, torch
        self.groups = []
        dev = next(iter(planes_src.values())).device
        passes = [(S, name, None) for S in luma_sizes for name in planes_src] + [(None, "Y", ts) for ts in rect_tx_sizes]
        for S, name, rect in passes:
            src = planes_src[name]
            side_h = None
            if rect is None:
                side = S if name == "Y" else S // 2
                if side < 4:
                    continue
                ts = TX_OF_SIDE[side]
            else:
                ts, side, side_h = rect, pkg.TX_W[rect], pkg.TX_H[rect]
            if src.dim() == 3:                # a stack of F pictures [F, H, W] (a GOP): every picture tiled on its own, one launch
                nf, ph, pw = src.shape
                if nf * ph > 0xffff:
                    raise ValueError("a stack of pictures must stay below 65 536 rows (16-bit origins)")
                xy1, offs1 = tile_origins(pw, ph, side, side_h)
                rows = (np.arange(nf, dtype=np.uint32) * np.uint32(ph))[:, None]
                xy = (xy1[None, :] + (rows << 16)).reshape(-1).astype(np.uint32)
                offs = (offs1[None, :] + rows * np.uint32(pw)).reshape(-1).astype(np.uint32)
            else:
                ph, pw = src.shape
                xy, offs = tile_origins(pw, ph, side, side_h)
            n = xy.size
            if n == 0:
                continue
            tt = (tx_types or {}).get(side, 0) if rect is None else 0
            _, iscan = pkg.tables.scan_tables(ts, tt)
            nc = min(side, 32) * min(side_h or side, 32)
            pred = planes_pred[name]
            recon = pred.clone()              # samples outside the full tiles keep the prediction, as in-place reconstruction would
            # 2-D planes may be views into padded picture buffers (PictureInput): their own row strides; the stack form is dense
            sst = src.stride(0) if src.dim() == 2 else pw
            pst = pred.stride(0) if pred.dim() == 2 else pw
            g = {"name": name, "luma_size": S if rect is None else f"{side}x{side_h}", "tx_size": ts, "tx_type": tt, "src": src, "src_stride": sst, "pred": pred, "pred_stride": pst,
                 "recon": recon, "recon_stride": pw, "xy": torch.from_numpy(xy.view(np.int32)).to(dev),
                 "offsets": torch.from_numpy(offs.view(np.int32)).to(dev) if ts == 0 else None,
                 "iscan": torch.from_numpy(iscan).to(dev), "qcoeff": torch.empty((n, nc), dtype=torch.int32, device=dev),
                 "eob": torch.zeros(n, dtype=torch.int16, device=dev), "pixels": n * side * (side_h or side)}
            if keep_coeff:
                g["coeff"] = torch.empty((n, nc), dtype=torch.int32, device=dev)
                g["dqcoeff"] = torch.empty((n, nc), dtype=torch.int32, device=dev)
            self.groups.append(g)
        # Placement: the two arrays a group's kernel writes at the same time - qcoeff and recon - are kept apart in device
        # memory: every group's qcoeff first, a temporary 32 GiB spacer, then every group's reconstruction (was: interleaved, group by group)
        if spread_outputs and self.groups and dev.type == "cuda":
            recon_src = [(g["recon"], g) for g in self.groups]
            for g in self.groups:
                g["recon"] = None
            del g
            qshapes = [tuple(g["qcoeff"].shape) for g in self.groups]
            for g in self.groups:
                g["qcoeff"] = None
            torch.cuda.empty_cache()
            spacers = []

            def gap():
                try:
                    spacers.append(torch.empty(32 << 30, dtype=torch.uint8, device=dev))
                except RuntimeError:
                    pass
            if spread_outputs == "all":          # the source and prediction planes too: [src] gap [pred] gap [qcoeff] gap [recon]
                for key in ("src", "pred"):
                    fresh = {}
                    for g in self.groups:
                        t0 = g[key]
                        if id(t0) not in fresh:
                            fresh[id(t0)] = t0.clone()
                        g[key] = fresh[id(t0)]
                    gap()
            for g, shp in zip(self.groups, qshapes):
                g["qcoeff"] = torch.empty(shp, dtype=torch.int32, device=dev)
            gap()
            for old_recon, g in recon_src:
                g["recon"] = old_recon.clone()
            del recon_src, old_recon, spacers
            torch.cuda.empty_cache()
        self.groups.sort(key=lambda g: g["name"] != "Y")      # luma groups first (stable): svt_hip_encode_recon_frame_ex's two phases
        self.n_luma = sum(g["name"] == "Y" for g in self.groups)
        self.array = dsp.make_frame_groups(self.groups)
        self.cfl_groups, self.cfl_array, self.levels_array = [], None, None
        self.is_16bit = is_16bit
        self.pixels = sum(g["pixels"] for g in self.groups)
        self.blocks = sum(g["xy"].numel() for g in self.groups)

    def run(self, qrow):
        """every group in one call (concurrent on the library's internal streams)"""
        self.dsp.encode_recon_frame(self.array, qrow, is_16bit=self.is_16bit, bd=10 if self.is_16bit else 8)

    def add_levels(self, fill=None):
        """one padded level buffer per block of every group (av1_txb_init_levels' levels_buf), 16-byte-aligned pitch"""
        t = self.torch
        for g in self.groups:
            w, h = min(self._side(g)[0], 32), min(self._side(g)[1], 32)
            pitch = ((w + 4) * (h + 6) + 16 + 15) // 16 * 16
            n = g["xy"].numel()
            g["levels"] = t.empty((n, pitch), dtype=t.uint8, device=g["xy"].device) if fill is None else \
                t.full((n, pitch), fill, dtype=t.uint8, device=g["xy"].device)
        self.levels_array = self.dsp.make_frame_levels([g["levels"] for g in self.groups])

    def _side(self, g):
        from . import TX_W, TX_H
        return TX_W[g["tx_size"]], TX_H[g["tx_size"]]

    def add_cfl(self, alpha_cb, alpha_cr, xy=None):
        """chroma-from-luma prediction for the chroma blocks of a pass with ONE luma size: alpha_* int32 per chroma block (of xy, default:
        every block of the Cb group); the luma reconstruction is the Y group's, the chroma predictions are predicted in place"""
        ys = [g for g in self.groups if g["name"] == "Y"]
        cs = [g for g in self.groups if g["name"] != "Y"]
        if len(ys) != 1 or len(cs) != 2 or ys[0]["recon"].dim() != 2:
            raise ValueError("add_cfl takes a pass with one luma size over one 4:2:0 picture")
        cw, ch = self._side(cs[0])
        self.cfl_groups = [{"luma_recon": ys[0]["recon"], "luma_stride": ys[0]["recon_stride"], "pred_cb": cs[0]["pred"], "cb_stride": cs[0]["pred_stride"],
                            "pred_cr": cs[1]["pred"], "cr_stride": cs[1]["pred_stride"], "xy": cs[0]["xy"] if xy is None else xy,
                            "alpha_cb": alpha_cb, "alpha_cr": alpha_cr, "width": cw, "height": ch}]
        self.cfl_array = self.dsp.make_frame_cfl_groups(self.cfl_groups)

    def run_ex(self, qrow):
        """luma groups -> chroma-from-luma prediction (add_cfl) -> chroma groups -> level maps (add_levels): one call"""
        self.dsp.encode_recon_frame_ex(self.array, qrow, self.n_luma, self.cfl_array, len(self.cfl_groups), self.levels_array,
                                       is_16bit=self.is_16bit, bd=10 if self.is_16bit else 8)

    def run_sequential(self, qrow):
        """the same groups, one entry-point call after the other on the caller's stream (what round 1 measured; the wrappers
        allocate their outputs from torch's caching allocator)"""
        d = self.dsp
        bd = 10 if self.is_16bit else 8
        for g in self.groups:
            d.encode_recon_planes(g["src"], g["src_stride"], g["pred"], g["pred_stride"], g["recon"], g["recon_stride"], g["xy"],
                                  g["tx_size"], g["tx_type"], qrow, g["iscan"], bd=bd)

    def digest(self):
        """int64 [blocks, sum eob, sum |qcoeff| weighted checksum, sum recon samples] of the pass, computed on the device"""
        t = self.torch
        d = t.zeros(4, dtype=t.int64, device=self.groups[0]["eob"].device)
        for g in self.groups:
            d[0] += g["xy"].numel()
            d[1] += (g["eob"].to(t.int64) & 0xffff).sum()
            q = g["qcoeff"].to(t.int64)
            w = (t.arange(q.shape[1], device=q.device, dtype=t.int64) % 8191) + 1
            d[2] += (q * w).sum() % DIGEST_MOD           # exact int64 sum (< 2^58), then the small residue
            d[3] += (g["recon"].to(t.int64) & 0xffff).sum()
        d[2] %= DIGEST_MOD
        return d


class PictureInput:
    """The picture-input side: frames of a y4m file -> the encoder's padded plane buffers in HBM, plus the 1/4 and
    1/16 luma pictures the hierarchical motion estimation searches.  Reference flow: ReadInputFrames (EbAppProcessCmd.c:765-900) ->
    CopyApiFromApp into the input EbPictureBufferDesc -> PadPictureToMultipleOfMinCuSizeDimensions / ...OfLcuDimensions and
    DecimateInputPicture (EbPictureAnalysisProcess.c:4818-4958).

    MI355X form: two pinned host staging buffers and two device staging buffers; frame k + 1 is read from the file and copied to
    the device on a copy stream while frame k's import / decimation kernels (and whatever the caller enqueues after them) run on
    the compute stream.  A 10-bit picture is kept as 16-bit samples (what the reference's own 16-bit DSP functions take after it
    packs its 8-bit + 2-bit planes), not as the split planes.  geometry: origin = border on every side (the reference's
    left / top padding), pad_right / pad_bottom = extension to a multiple of the minimum CU size (8)."""

    def __init__(self, dsp, pkg, path, origin=(64 + 4, 64 + 4), min_cu=8, with_decimation=True, device="cuda:0"):
        torch = dsp.torch
        self.dsp, self.t = dsp, torch
        self.rd = pkg.Y4mReader(dsp.lib, path)
        i = self.rd.info
        if i.chroma != b"420" or i.bit_depth not in (8, 10):
            self.rd.close()
            raise pkg.SvtHipError(f"PictureInput handles 4:2:0 at 8 or 10 bits (file: {i.chroma.decode()} / {i.bit_depth})")
        self.w, self.h, self.is16 = i.width, i.height, i.bit_depth > 8
        self.pad_right = (-self.w) % min_cu
        self.pad_bottom = (-self.h) % min_cu
        self.ox, self.oy = origin
        self.W, self.H = self.w + self.pad_right, self.h + self.pad_bottom
        dt = torch.int16 if self.is16 else torch.uint8
        nsamp = self.rd.frame_bytes // (2 if self.is16 else 1)
        self.host = [torch.empty(nsamp, dtype=dt).pin_memory() for _ in range(2)]
        self.stage = [torch.empty(nsamp, dtype=dt, device=device) for _ in range(2)]
        self.copy_stream = torch.cuda.Stream(device=device)
        self.copied = [torch.cuda.Event() for _ in range(2)]
        self.consumed = [torch.cuda.Event() for _ in range(2)]

        def plane(w, h, ox, oy):
            stride = (w + 2 * ox + 63) & ~63
            return torch.empty((h + 2 * oy, stride), dtype=dt, device=device)
        self.planes = (plane(self.W, self.H, self.ox, self.oy), plane(self.W >> 1, self.H >> 1, self.ox >> 1, self.oy >> 1),
                       plane(self.W >> 1, self.H >> 1, self.ox >> 1, self.oy >> 1))
        self.quarter = self.sixteenth = None
        # a deeper picture's analysis plane: its samples' top 8 bits (what the reference's HME / ME / intra search read), same geometry
        self.luma8 = torch.empty(self.planes[0].shape, dtype=torch.uint8, device=device) if self.is16 else None
        self.bd = i.bit_depth
        if with_decimation:
            self.q_origin = (self.ox >> 1, self.oy >> 1)
            self.s_origin = (self.ox >> 2, self.oy >> 2)
            qw, qh, sw, sh = (self.W + 1) // 2, (self.H + 1) // 2, (self.W + 3) // 4, (self.H + 3) // 4
            self.quarter = torch.empty((qh + 2 * self.q_origin[1], (qw + 2 * self.q_origin[0] + 63) & ~63), dtype=torch.uint8, device=device)
            self.sixteenth = torch.empty((sh + 2 * self.s_origin[1], (sw + 2 * self.s_origin[0] + 63) & ~63), dtype=torch.uint8, device=device)
        self.slot = 0
        self.pending = self._fetch(0)

    def _fetch(self, slot):
        """read the next frame into pinned buffer `slot` and start its copy to the device; False at the end of the file"""
        self.consumed[slot].synchronize()                 # the import kernel that read this device buffer has finished
        if not self.rd.read_into(self.host[slot].numpy()):
            return False
        with self.t.cuda.stream(self.copy_stream):
            self.stage[slot].copy_(self.host[slot], non_blocking=True)
            self.copied[slot].record(self.copy_stream)
        return True

    def next(self):
        """-> (y, cb, cr) padded planes of the next frame (enqueued on the current stream), or None at the end of the file.  The
        planes are overwritten by the following call."""
        if not self.pending:
            return None
        slot = self.slot
        cur = self.t.cuda.current_stream()
        cur.wait_event(self.copied[slot])
        self.dsp.picture_import(self.stage[slot], self.w, self.h, self.planes, self.ox, self.oy, self.pad_right, self.pad_bottom)
        self.consumed[slot].record(cur)
        if self.luma8 is not None:
            self.dsp.picture_luma8(self.planes[0], self.luma8, self.W + 2 * self.ox, self.H + 2 * self.oy, self.bd)
        if self.quarter is not None:
            y = self.luma8 if self.luma8 is not None else self.planes[0]
            self.dsp.picture_decimate(y[self.oy:, self.ox:], y.stride(0), self.W, self.H, self.quarter, self.q_origin, self.sixteenth, self.s_origin)
        self.slot ^= 1
        self.pending = self._fetch(self.slot)             # overlaps with the kernels just enqueued
        return self.planes

    def close(self):
        self.rd.close()
