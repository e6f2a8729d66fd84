"""GPU: BASELINE.json configs[3] and configs[4] as parity cases.

C4  full 1080p yuv420p frame, every CU size: residual -> FwdTxfm2d -> quant -> dequant ->
    InvTxfm2d + add, recon bit-exact vs the CPU oracle.
C5  4k 10-bit sequence sharded per GOP: here a reduced sequence on one GPU walks the same
    per-GOP code path (bd = 10 kernels, GOP -> rank map); the 8-GPU run only changes which
    rank owns which GOP (tests/test_dist_cpu.py covers the 2-rank exchange on gloo)."""
import ctypes

import numpy as np
import pytest
import torch

import svtlibs
from poison import poisoned_outputs  # noqa: F401
from svtlibs import TX_H, TX_W, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def roundtrip_plane(dsp, src, pred, tx_size, qrow, bd, sample_step):
    """GPU round trip of one plane tiled with tx_size blocks; returns (recon, checked)"""
    O = svtlibs.oracle()
    ph, pw = src.shape
    w, h = TX_W[tx_size], TX_H[tx_size]
    xs = np.arange(0, pw - w + 1, w); ys = np.arange(0, ph - h + 1, h)
    xy = np.array([(y << 16) | x for y in ys for x in xs], np.uint32)
    offs = np.array([y * pw + x for y in ys for x in xs], np.uint32)
    _, iscan = svtlibs.scan_tables(tx_size, 0)
    is8 = bd == 8
    as_dev = (lambda a: dev(a)) if is8 else (lambda a: dev(a.view(np.int16)))
    d_src, d_pred = as_dev(src), as_dev(pred)
    co, q, dq, eob, _, _ = dsp.fwd_quant_planes(d_src, pw, d_pred, pw, dev(xy.view(np.int32)), tx_size, 0, qrow, dev(iscan), bd=bd)
    recon = d_pred.clone()
    dsp.inv_txfm2d_add(dq, recon, tx_size, 0, bd, dst_stride=pw, dst_block_pitch=0, offsets=dev(offs.view(np.int32)))
    torch.cuda.synchronize()
    rec = recon.cpu().numpy()
    rec = rec if is8 else rec.view(np.uint16)
    qh = q.cpu().numpy(); eobh = eob.cpu().numpy().view(np.uint16)
    checked = 0
    for i in range(0, len(xy), sample_step):
        y, x = int(xy[i] >> 16), int(xy[i] & 0xffff)
        rc = np.zeros(1024, np.int32); rq = np.zeros(1024, np.int32); rdq = np.zeros(1024, np.int32)
        reob = np.zeros(1, np.uint16)
        sp = ctypes.c_void_p(src.ctypes.data + (y * pw + x) * src.itemsize)
        pp = ctypes.c_void_p(pred.ctypes.data + (y * pw + x) * pred.itemsize)
        O.svt_oracle_fwd_quant_planes(sp, pw, pp, pw, int(not is8), bd, tx_size, 0, ptr(qrow["zbin"]), ptr(qrow["round"]),
                                      ptr(qrow["quant"]), ptr(qrow["quant_shift"]), ptr(qrow["dequant"]), ptr(rc), ptr(rq),
                                      ptr(rdq), ptr(reob), None, None)
        blk = np.ascontiguousarray(pred[y:y + h, x:x + w]).astype(np.uint16)
        O.svt_oracle_inv_txfm2d_add(ptr(rdq), ptr(blk), w, 0, tx_size, bd)
        assert np.array_equal(rec[y:y + h, x:x + w].astype(np.uint16), blk), (tx_size, x, y)
        assert np.array_equal(qh[i], rq[:qh.shape[1]]) and eobh[i] == reob[0]
        checked += 1
    # untouched margin (when the plane is not a multiple of the block size) must equal pred
    if pw % w:
        assert np.array_equal(rec[:, (pw // w) * w:], pred[:, (pw // w) * w:])
    if ph % h:
        assert np.array_equal(rec[(ph // h) * h:, :], pred[(ph // h) * h:, :])
    return rec, checked


def test_config4_1080p_all_cu_sizes_roundtrip(dsp):
    rng = np.random.default_rng(13596)
    qt = svtlibs.quant_tables(8)
    qrow = {k: v[100].copy() for k, v in qt.items()}
    y_src = rng.integers(0, 256, size=(1080, 1920), dtype=np.uint8)
    y_pred = np.clip(y_src.astype(int) + rng.integers(-40, 41, size=y_src.shape), 0, 255).astype(np.uint8)
    c_src = rng.integers(0, 256, size=(540, 960), dtype=np.uint8)
    c_pred = rng.integers(0, 256, size=(540, 960), dtype=np.uint8)
    total = 0
    for tx_size, want_blocks, step in ((4, 480, 7), (3, 1980, 23), (2, 8040, 97), (1, 32400, 397), (0, 129600, 1571)):
        w = TX_W[tx_size]
        assert (1920 // w) * (1080 // w) == want_blocks          # SURVEY §8d block counts
        _, n = roundtrip_plane(dsp, y_src, y_pred, tx_size, qrow, 8, step)
        total += n
    for tx_size, step in ((3, 11), (2, 53), (1, 211), (0, 797)):   # chroma 960x540, sizes S/2 >= 4
        _, n = roundtrip_plane(dsp, c_src, c_pred, tx_size, qrow, 8, step)
        total += n
    assert total > 500


def test_config5_10bit_gop_shards_single_gpu(dsp, pkg):
    from cidana_svt_av1_amd import sharding
    rng = np.random.default_rng(13597)
    qt = svtlibs.quant_tables(10)
    qrow = {k: v[120].copy() for k, v in qt.items()}
    n_gops, frames_per_gop, world = 4, 2, 8
    digests = []
    for g in range(n_gops):
        assert sharding.gop_owner(g, world) == g
        for f in range(frames_per_gop):
            src = rng.integers(0, 1024, size=(128, 256)).astype(np.uint16)
            pred = np.clip(src.astype(int) + rng.integers(-64, 65, size=src.shape), 0, 1023).astype(np.uint16)
            for tx_size, step in ((4, 1), (3, 3), (1, 37)):
                rec, n = roundtrip_plane(dsp, src, pred, tx_size, qrow, 10, step)
                assert n > 0 and rec.max() <= 1023
                digests.append(int(rec.astype(np.int64).sum()))
    assert len(digests) == n_gops * frames_per_gop * 3
