"""GPU: svt_hip_intra_fast_loop_frame (the intra candidates of the mode-decision fast loop, fused) against the reference's own
results (tests/golden/fast_loop.npz), against the composed library path at scale (svt_hip_build_intra_predictors_batch per candidate,
which tests/test_gpu_bip.py pins to the reference, then the distortion in torch) with an oracle spot check, and as the first stage of
the fast loop -> full loop chain.  Every output tensor starts filled with a sentinel."""
import ctypes
import os

import numpy as np
import pytest
import torch

import svtlibs
from svtlibs import TX_H, TX_W, ptr

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PITCH = 1 + 2 * 64 + 15
SENT = 0x5a5a5a5a5a5a5a5a
SAD, SSD = 0, 1
C_FL, AVX2 = 0, 1
ERR_INVALID = -2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinel_dist(n, c):
    return torch.full((n, c), SENT, dtype=torch.int64, device="cuda")


def list_of(s):
    w, h = TX_W[s], TX_H[s]
    nd = 1 if (w, h) in ((4, 4), (4, 8), (8, 4)) else 7
    modes, deltas = [], []
    for m in range(13):
        for k in (range(nd) if 1 <= m <= 8 else range(1)):
            modes.append(m); deltas.append(0 if nd == 1 or not 1 <= m <= 8 else k - 3)
    return modes, deltas


def rand_case(rng, s, n):
    """n random blocks of size s: edges uint8 [n, PITCH] (element 0 = corner), descriptors uint8 [n, 8], dense source [n, H, W]"""
    w, h = TX_W[s], TX_H[s]
    top = rng.integers(0, 256, (n, PITCH)).astype(np.uint8); left = rng.integers(0, 256, (n, PITCH)).astype(np.uint8)
    flat = rng.random(n) < 0.2                                  # flat neighbourhoods: ties in PAETH, equal DC sums
    top[flat] = top[flat, :1]; left[flat] = top[flat, :1]
    n_top = np.where(rng.random(n) < 0.15, 0, np.where(rng.random(n) < 0.7, w, rng.integers(1, w // 4 + 1, n) * 4))
    n_left = np.where(rng.random(n) < 0.15, 0, np.where(rng.random(n) < 0.7, h, rng.integers(1, h // 4 + 1, n) * 4))
    n_tr = np.where(n_top == w, rng.choice([0, h, -1], n), 0); n_tr = np.where(n_tr < 0, rng.integers(0, h + 1, n), n_tr)
    n_bl = np.where(n_left == h, rng.choice([0, w, -1], n), 0); n_bl = np.where(n_bl < 0, rng.integers(0, w + 1, n), n_bl)
    blk = np.stack([np.zeros(n), np.zeros(n), rng.integers(0, 2, n), rng.random(n) < 0.2, n_top, n_tr, n_left, n_bl], 1).astype(np.uint8)
    src = rng.integers(0, 256, (n, h, w)).astype(np.uint8)
    wide = rng.random(n) < 0.1                                  # large residuals: the wrapped difference
    src[wide] = 255
    top[wide] = rng.integers(0, 4, (int(wide.sum()), PITCH)); left[wide] = rng.integers(0, 4, (int(wide.sum()), PITCH))
    return top, left, blk, src


def composed(dsp, s, top_d, left_d, blk, modes, deltas):
    """predictions [n, C, H, W] from svt_hip_build_intra_predictors_batch, one batch per candidate"""
    preds = []
    for m, a in zip(modes, deltas):
        b = blk.copy(); b[:, 0] = m; b[:, 1] = np.uint8(a & 0xff)
        preds.append(dsp.build_intra_predictors(top_d, left_d, dev(b), s))
    return torch.stack(preds, 1)


def dist_of(src_d, pred, metric, flavour):
    """src [n, H, W], pred [n, C, H, W] -> [n, C] int64, one candidate at a time"""
    out = []
    for c in range(pred.shape[1]):
        d = src_d.to(torch.int32) - pred[:, c].to(torch.int32)
        if metric == SAD:
            out.append(d.abs().sum((1, 2), dtype=torch.int64))
            continue
        if flavour == AVX2:
            t = d & 255
            d = torch.where(t <= 128, t, 256 - t)
        out.append((d * d).sum((1, 2), dtype=torch.int64))
    return torch.stack(out, 1)


def to_plane(src, cols=64):
    """dense blocks [n, H, W] -> a plane with the blocks on a grid at odd origins, its stride, and xy = x | y << 16"""
    n, h, w = src.shape
    rows = (n + cols - 1) // cols
    stride = cols * (w + 1) + 3
    plane = np.zeros((rows * (h + 1) + 1, stride), np.uint8)
    xy = np.zeros(n, np.uint32)
    for i in range(n):
        y, x = 1 + (i // cols) * (h + 1), 1 + (i % cols) * (w + 1)
        plane[y:y + h, x:x + w] = src[i]
        xy[i] = x | y << 16
    return plane, stride, xy


def test_fixture_parity_every_size_metric_and_flavour(dsp):
    g = np.load(os.path.join(G, "fast_loop.npz"))
    runs = 0
    for s in range(19):
        p = f"s{s}_"
        modes, deltas = [int(v) for v in g[p + "modes"]], [int(v) for v in g[p + "deltas"]]
        top, left = dev(g[p + "top"][:, 15:15 + PITCH]), dev(g[p + "left"][:, 15:15 + PITCH])
        blk, src = dev(g[p + "blk"]), dev(g[p + "src"])
        for metric, flavour, key in ((SAD, C_FL, "sad"), (SAD, AVX2, "sad"), (SSD, C_FL, "ssd_c"), (SSD, AVX2, "ssd_avx2")):
            if p + key not in g.files:
                continue
            dist, _ = dsp.intra_fast_loop(src, top, left, blk, s, modes, deltas, metric, flavour)
            assert np.array_equal(dist.cpu().numpy().astype(np.uint64), g[p + key]), (s, key, flavour)
            runs += 1
    assert runs == 19 * 3 + 5


@pytest.mark.parametrize("s", range(19))
def test_random_blocks_at_scale_vs_composed_path_and_oracle(dsp, s):
    """2^14 random blocks with random availability and the full list; SAD on a dense source, SSD (C) on a plane-addressed one, the
    wrapped SSD (AVX2) on square sizes; 8 blocks also through the CPU oracle"""
    rng = np.random.default_rng(1152 + s)
    w, h = TX_W[s], TX_H[s]
    n = 1 << 14
    top, left, blk, src = rand_case(rng, s, n)
    modes, deltas = list_of(s)
    top_d, left_d, src_d = dev(top), dev(left), dev(src)
    pred = composed(dsp, s, top_d, left_d, blk, modes, deltas)
    blk_d = dev(blk)
    got, _ = dsp.intra_fast_loop(src_d, top_d, left_d, blk_d, s, modes, deltas, SAD)
    assert torch.equal(got, dist_of(src_d, pred, SAD, C_FL)), s
    plane, stride, xy = to_plane(src)
    got, _ = dsp.intra_fast_loop(dev(plane), top_d, left_d, blk_d, s, modes, deltas, SSD, C_FL, src_xy=dev(xy.view(np.int32)), src_stride=stride)
    ssd_c = dist_of(src_d, pred, SSD, C_FL)
    assert torch.equal(got, ssd_c), s
    if w == h:
        got, _ = dsp.intra_fast_loop(src_d, top_d, left_d, blk_d, s, modes, deltas, SSD, AVX2)
        assert torch.equal(got, dist_of(src_d, pred, SSD, AVX2)), s
    O = svtlibs.oracle()
    ssd_c = ssd_c.cpu().numpy()
    for i in rng.choice(n, 8, replace=False):
        t = np.zeros(15 + PITCH, np.uint8); t[15:] = top[i]; l_ = np.zeros(15 + PITCH, np.uint8); l_[15:] = left[i]
        for c, (m, a) in enumerate(zip(modes, deltas)):
            o = np.zeros((h, w), np.uint8)
            O.svt_oracle_build_intra_predictors(0, ctypes.c_void_p(t.ctypes.data + 16), ctypes.c_void_p(l_.ctypes.data + 16), ptr(o), w, m, a, s,
                                                int(blk[i, 3]), int(blk[i, 4]), int(blk[i, 5]), int(blk[i, 6]), int(blk[i, 7]), int(blk[i, 2]), 8)
            dd = src[i].astype(np.int64) - o
            assert int((dd * dd).sum()) == int(ssd_c[i, c]), (s, i, c)


def test_several_groups_in_one_call_and_predictions(dsp):
    """groups of different sizes (and an empty one) in one call == each group alone; d_pred == the composed path's predictions when
    asked for, a sentinel buffer that is not passed stays as it is"""
    rng = np.random.default_rng(77)
    groups, refs, keep = [], [], []
    for s, n in ((0, 3000), (4, 70), (9, 600), (13, 1000), (16, 200), (2, 0)):
        top, left, blk, src = rand_case(rng, s, max(n, 1))
        modes, deltas = list_of(s)
        if s == 9:
            modes, deltas = modes[:13], deltas[:13]
        top_d, left_d, src_d, blk_d = dev(top), dev(left), dev(src), dev(blk)
        dist = sentinel_dist(max(n, 1), len(modes))
        pred = torch.full((max(n, 1), len(modes), TX_H[s], TX_W[s]), 0x5a, dtype=torch.uint8, device="cuda")
        groups.append(dict(src=src_d, top=top_d, left=left_d, blocks=blk_d, nblocks=n, tx_size=s, modes=modes, deltas=deltas, dist=dist,
                           pred=pred if s != 4 else None))
        keep.append(pred)
        refs.append(composed(dsp, s, top_d, left_d, blk, modes, deltas) if n else None)
    assert dsp.intra_fast_loop_frame(groups, SSD, C_FL) == 0
    torch.cuda.synchronize()
    for g, r, pbuf in zip(groups, refs, keep):
        if r is None:
            assert (g["dist"] == SENT).all()
            continue
        assert torch.equal(g["dist"], dist_of(g["src"], r, SSD, C_FL)), g["tx_size"]
        if g["pred"] is not None:
            assert torch.equal(g["pred"], r), g["tx_size"]
        else:
            assert (pbuf == 0x5a).all(), "prediction written without being asked for"


@pytest.mark.parametrize("s", [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 13, 14, 15, 16])
def test_chroma_cb_plus_cr_equals_oracle(dsp, s):
    """CHROMA_MODE_0 with a UV mode other than CfL: the same distortion on Cb and on Cr (chroma sizes 4 .. 32), summed"""
    rng = np.random.default_rng(900 + s)
    w, h = TX_W[s], TX_H[s]
    n = 24
    modes, deltas = list(range(13)), [0] * 13                    # UV_DC_PRED .. UV_PAETH_PRED, angle_delta[PLANE_TYPE_UV] = 0
    O = svtlibs.oracle()
    for metric in (SAD, SSD):
        tot = np.zeros((n, 13), np.int64)
        outs = []
        for plane in range(2):
            top, left, blk, src = rand_case(rng, s, n)
            d, _ = dsp.intra_fast_loop(dev(src), dev(top), dev(left), dev(blk), s, modes, deltas, metric, C_FL)
            outs.append(d)
            for i in range(n):
                t = np.zeros(15 + PITCH, np.uint8); t[15:] = top[i]; l_ = np.zeros(15 + PITCH, np.uint8); l_[15:] = left[i]
                for c in range(13):
                    o = np.zeros((h, w), np.uint8)
                    O.svt_oracle_build_intra_predictors(0, ctypes.c_void_p(t.ctypes.data + 16), ctypes.c_void_p(l_.ctypes.data + 16), ptr(o), w, c,
                                                        0, s, int(blk[i, 3]), int(blk[i, 4]), int(blk[i, 5]), int(blk[i, 6]), int(blk[i, 7]),
                                                        int(blk[i, 2]), 8)
                    dd = src[i].astype(np.int64) - o
                    tot[i, c] += int(np.abs(dd).sum()) if metric == SAD else int((dd * dd).sum())
        assert np.array_equal((outs[0] + outs[1]).cpu().numpy(), tot), (s, metric)


def test_chain_fast_loop_then_full_loop(dsp, pkg):
    """fast loop (SSD) -> each block's best candidate -> its d_pred -> svt_hip_full_loop_frame == the same chain from the composed
    predictions"""
    rng = np.random.default_rng(4242)
    s, n = 2, 4096                                              # 16x16
    top, left, blk, src = rand_case(rng, s, n)
    src = np.clip(top[:, 1:17][:, None, :].astype(np.int64) + rng.integers(-6, 7, (n, 16, 16)), 0, 255).astype(np.uint8)
    modes, deltas = list_of(s)
    top_d, left_d, src_d, blk_d = dev(top), dev(left), dev(src), dev(blk)
    dist, pred = dsp.intra_fast_loop(src_d, top_d, left_d, blk_d, s, modes, deltas, SSD, C_FL, want_pred=True)
    ref = composed(dsp, s, top_d, left_d, blk, modes, deltas)
    ref_dist = dist_of(src_d, ref, SSD, C_FL)
    best = torch.argmin(dist, 1)                                 # first minimum, as the reference's sort keeps the list order on ties
    assert torch.equal(best, torch.argmin(ref_dist, 1))
    ar = torch.arange(n, device="cuda")
    qt = svtlibs.quant_tables(8)
    qrow = {k: v[120].copy() for k, v in qt.items()}
    a = dsp.full_loop(src_d, pred[ar, best].contiguous(), s, [0, 1, 2, 3], qrow, flavour=1)
    b = dsp.full_loop(src_d, ref[ar, best].contiguous(), s, [0, 1, 2, 3], qrow, flavour=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_argument_validation_launches_nothing(dsp):
    rng = np.random.default_rng(5)
    top, left, blk, src = rand_case(rng, 8, 64)                  # 16x8
    base = dict(src=dev(src), top=dev(top), left=dev(left), blocks=dev(blk), nblocks=64, tx_size=8, modes=[0, 1, 9], deltas=[0, 2, 0])
    cases = [
        (dict(modes=[], deltas=[]), SAD, C_FL),                  # ncand 0
        (dict(ncand=65, modes=[0] * 64, deltas=[0] * 64), SAD, C_FL),
        (dict(modes=[0, 13, 9]), SAD, C_FL),                     # mode above 12
        (dict(deltas=[0, 4, 0]), SAD, C_FL),                     # delta outside -3..3
        (dict(deltas=[0, -4, 0]), SAD, C_FL),
        (dict(deltas=[1, 0, 0]), SAD, C_FL),                     # delta on DC
        (dict(deltas=[0, 0, -1]), SAD, C_FL),                    # delta on SMOOTH
        (dict(src=None), SAD, C_FL), (dict(top=None), SAD, C_FL), (dict(left=None), SAD, C_FL), (dict(blocks=None), SAD, C_FL),
        (dict(tx_size=19), SAD, C_FL), (dict(tx_size=-1), SAD, C_FL),
        ({}, SSD, AVX2),                                         # the wrapped SSD on 16x8
        ({}, 2, C_FL), ({}, SAD, 2),                             # metric / flavour
        (dict(neigh_pitch=16), SAD, C_FL),
    ]
    empty = dict(base, nblocks=0, tx_size=99, dist=sentinel_dist(1, 3))         # a garbage tx_size in an EMPTY group
    for over, metric, flavour in cases:
        dist = sentinel_dist(64, 3)
        g = dict(base, dist=dist)
        g.update(over)
        for groups in ([g], [dict(base, dist=sentinel_dist(64, 3)), g]):
            assert dsp.intra_fast_loop_frame(groups, metric, flavour) == ERR_INVALID, over
        torch.cuda.synchronize()
        assert (dist == SENT).all(), over
    ok = dict(base, dist=sentinel_dist(64, 3))
    assert dsp.intra_fast_loop_frame([ok, empty], SAD, C_FL) == ERR_INVALID          # the empty group's tx_size is checked too
    torch.cuda.synchronize()
    assert (ok["dist"] == SENT).all()
    bad = torch.empty(64 * 3 + 1, dtype=torch.int64, device="cuda")[1:].view(64, 3)
    pred = torch.empty(64 * 3 * 128 + 4, dtype=torch.uint8, device="cuda")[4:]
    assert dsp.intra_fast_loop_frame([dict(base, dist=dev(np.zeros((64, 3), np.int64)), pred=pred)], SAD, C_FL) == ERR_INVALID
    assert dsp.intra_fast_loop_frame([dict(base, dist=bad)], SAD, C_FL) == 0                         # 8-byte aligned: fine
    dist_u8 = torch.empty(64 * 3 * 8 + 4, dtype=torch.uint8, device="cuda")
    g = dict(base, dist=None)
    arr = dsp.make_fast_loop_groups([g])
    arr[0].d_dist = dist_u8.data_ptr() + 4                                                           # misaligned d_dist
    assert dsp.intra_fast_loop_frame(arr, SAD, C_FL) == ERR_INVALID
    assert dsp.intra_fast_loop_frame([], SAD, C_FL) == 0


def test_graph_capture_replays_the_same_result(dsp):
    rng = np.random.default_rng(9)
    s = 3
    top, left, blk, src = rand_case(rng, s, 2048)
    modes, deltas = list_of(s)
    dist = sentinel_dist(2048, len(modes))
    # the group table holds raw pointers: its tensors must outlive the graph (torch.cuda.graph empties the allocator's cache on entry)
    g = dict(src=dev(src), top=dev(top), left=dev(left), blocks=dev(blk), nblocks=2048, tx_size=s, modes=modes, deltas=deltas, dist=dist)
    groups = dsp.make_fast_loop_groups([g])
    assert dsp.intra_fast_loop_frame(groups, SSD, C_FL) == 0
    torch.cuda.synchronize()
    want = dist.clone()
    dist.fill_(SENT)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s_ = torch.cuda.Stream()
    with torch.cuda.stream(s_):
        with torch.cuda.graph(graph, stream=s_):
            rc = dsp.intra_fast_loop_frame(groups, SSD, C_FL)
    assert rc == 0
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dist, want)
