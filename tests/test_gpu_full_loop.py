"""GPU: svt_hip_full_loop_frame, the fused luma mode-decision full loop (residual -> transform -> quantiser -> distortion per block and
transform type), against the reference's fixture (tests/golden/full_loop.npz), the CPU oracle, and the library's own two-call path."""
import ctypes
import os

import numpy as np
import pytest
import torch

import layouts
import poison
import svtlibs
from svtlibs import TX_H, TX_W, ptr, txfm_allowed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "full_loop.npz")
SENT = 0x5a


def nc_of(s):
    return min(TX_W[s], 32) * min(TX_H[s], 32)


def allowed(s):
    return [t for t in range(16) if txfm_allowed(s, t)]


def iscans(s, types):
    return torch.from_numpy(np.stack([svtlibs.scan_tables(s, t)[1] for t in types])).to(DEV)


def outputs(n, s, T, want_coeffs=True):
    """output tensors filled with the 0x5a sentinel"""
    f = lambda shape, dt: torch.full(shape, 0, dtype=dt, device=DEV).view(torch.uint8).fill_(SENT).view(dt)
    o = {"dist": f((n, T, 2), torch.int64), "eob": f((n, T), torch.int16)}
    if want_coeffs:
        o["qcoeff"] = f((n, T, nc_of(s)), torch.int32)
        o["dqcoeff"] = f((n, T, nc_of(s)), torch.int32)
    return o


def qrow_of(q):
    return {k: np.ascontiguousarray(v[q]) for k, v in svtlibs.quant_tables(8).items()}


def run(dsp, groups, qrow, flavour):
    rc = dsp.full_loop_frame(groups, qrow, flavour)
    torch.cuda.synchronize()
    assert rc == 0, dsp.lib.svt_hip_last_error()


def test_golden_fixture_every_size_and_type(dsp):
    z = np.load(GOLD)
    for qi, q in enumerate(z["s0_qindex"]):
        qrow = qrow_of(int(q))
        for flavour, key in ((0, "dist_c"), (1, "dist_avx2")):
            groups, want = [], []
            for s in range(19):
                types = [int(t) for t in z[f"s{s}_types"]][::-1]          # an order other than the fixture's
                perm = [list(z[f"s{s}_types"]).index(t) for t in types]
                src = torch.from_numpy(z[f"s{s}_src"].reshape(-1, TX_H[s], TX_W[s])).to(DEV)
                pred = torch.from_numpy(z[f"s{s}_pred"].reshape(-1, TX_H[s], TX_W[s])).to(DEV)
                n = src.shape[0]
                o = outputs(n, s, len(types))
                groups.append(dict(src=src, pred=pred, nblocks=n, tx_size=s, tx_types=types, iscan=iscans(s, types), **o))
                want.append((s, perm))
            run(dsp, groups, qrow, flavour)
            for g, (s, perm) in zip(groups, want):
                T = len(perm)
                # fixture [T, q, input, block, ...] -> [input * block, T, ...] in the call's type order
                wd = z[f"s{s}_{key}"][perm, qi].reshape(T, -1, 2).transpose(1, 0, 2).astype(np.int64)
                we = z[f"s{s}_eob"][perm, qi].reshape(T, -1).T.astype(np.int16)
                wq = z[f"s{s}_qcoeff"][perm, qi].reshape(T, -1, nc_of(s)).transpose(1, 0, 2)
                wdq = z[f"s{s}_dqcoeff"][perm, qi].reshape(T, -1, nc_of(s)).transpose(1, 0, 2)
                assert np.array_equal(g["dist"].cpu().numpy(), wd), (s, int(q), key)
                assert np.array_equal(g["eob"].cpu().numpy(), we), (s, int(q))
                assert np.array_equal(g["qcoeff"].cpu().numpy(), wq), (s, int(q))
                assert np.array_equal(g["dqcoeff"].cpu().numpy(), wdq), (s, int(q))


@pytest.mark.parametrize("fill", poison.FILLS, ids=lambda f: f"fill{f:02X}")
def test_the_plane_form_with_source_and_prediction_laid_out_unlike_each_other_equals_the_fixture(dsp, fill):
    """the fixture's 8x8 and 16x32 blocks painted into one source and one prediction picture, eight to a row: src_stride unlike
    pred_stride (both odd), the two pictures at different places in allocations of different sizes (tests/layouts.py asserts that a
    mix-up of the two stays inside them); one group per size, both flavours, against the fixture"""
    z = np.load(GOLD)
    sizes = (1, next(i for i in range(19) if (TX_W[i], TX_H[i]) == (16, 32)))
    blocks = {s: (z[f"s{s}_src"].reshape(-1, TX_H[s], TX_W[s]), z[f"s{s}_pred"].reshape(-1, TX_H[s], TX_W[s])) for s in sizes}
    PW = 8 * 16
    bands = [-(-len(blocks[s][0]) // 8) * TX_H[s] for s in sizes]
    srcp, predp, xy, y0 = np.zeros((sum(bands), PW), np.uint8), np.zeros((sum(bands), PW), np.uint8), {}, 0
    for s, band in zip(sizes, bands):
        w, h = TX_W[s], TX_H[s]
        pos = [((i % 8) * w, y0 + (i // 8) * h) for i in range(len(blocks[s][0]))]
        for (x, y), sb, pb in zip(pos, *blocks[s]):
            srcp[y:y + h, x:x + w], predp[y:y + h, x:x + w] = sb, pb
        xy[s] = np.array([x | (y << 16) for x, y in pos], np.int32)
        y0 += band
    spec = layouts.CallSpec("svt_hip_full_loop_frame", [layouts.Plane(n, PW, srcp.shape[0], stacked=False) for n in ("src", "pred")])
    lay = layouts.distinct_layouts(spec)
    with poison.poisoned(dsp, fill):
        (d_src,), p_src = layouts.place_operand(spec, lay, "src", [srcp], 1, fill)
        (d_pred,), p_pred = layouts.place_operand(spec, lay, "pred", [predp], 1, fill)
        assert d_src.stride(0) != d_pred.stride(0) and d_src.stride(0) % 2 and d_pred.stride(0) % 2
        for qi, q in enumerate(z["s0_qindex"]):
            for flavour, key in ((0, "dist_c"), (1, "dist_avx2")):
                groups = []
                for s in sizes:
                    types = [int(t) for t in z[f"s{s}_types"]]
                    groups.append(dict(src=d_src, src_stride=d_src.stride(0), src_xy=torch.from_numpy(xy[s]).to(DEV), pred=d_pred,
                                       pred_stride=d_pred.stride(0), pred_xy=torch.from_numpy(xy[s]).to(DEV), nblocks=len(xy[s]), tx_size=s,
                                       tx_types=types, iscan=iscans(s, types), **outputs(len(xy[s]), s, len(types))))
                run(dsp, groups, qrow_of(int(q)), flavour)
                for g, s in zip(groups, sizes):
                    T = len(g["tx_types"])
                    assert np.array_equal(g["dist"].cpu().numpy(), z[f"s{s}_{key}"][:, qi].reshape(T, -1, 2).transpose(1, 0, 2).astype(np.int64)), (s, int(q), key)
                    assert np.array_equal(g["eob"].cpu().numpy(), z[f"s{s}_eob"][:, qi].reshape(T, -1).T.astype(np.int16)), (s, int(q))
                    assert np.array_equal(g["qcoeff"].cpu().numpy(), z[f"s{s}_qcoeff"][:, qi].reshape(T, -1, nc_of(s)).transpose(1, 0, 2)), (s, int(q))
                    assert np.array_equal(g["dqcoeff"].cpu().numpy(), z[f"s{s}_dqcoeff"][:, qi].reshape(T, -1, nc_of(s)).transpose(1, 0, 2)), (s, int(q))
        layouts.assert_all_intact(p_src + p_pred, fill)


def oracle_chain(O, s, t, qrow, src_blk, pred_blk, iscan_np):
    """the per-block reference chain on the CPU oracle: (dist_c, dist_avx2, eob, qcoeff, dqcoeff)"""
    w, h = TX_W[s], TX_H[s]
    n = nc_of(s)
    co = np.zeros(n, np.int32); q = np.zeros(n, np.int32); dq = np.zeros(n, np.int32)
    eob = np.zeros(1, np.uint16); en = np.zeros(1, np.uint64)
    a = np.ascontiguousarray(src_blk); b = np.ascontiguousarray(pred_blk)
    O.svt_oracle_fwd_quant_planes(ptr(a), w, ptr(b), w, 0, 8, s, t, ptr(qrow["zbin"]), ptr(qrow["round"]), ptr(qrow["quant"]),
                                  ptr(qrow["quant_shift"]), ptr(qrow["dequant"]), ptr(co), ptr(q), ptr(dq), ptr(eob), None, ptr(en))
    kw, kh = min(w, 32), min(h, 32)
    pels = w * h
    sh = 2 if pels <= 256 else (0 if pels <= 1024 else -2)
    res = []
    for fn in (O.svt_oracle_full_distortion32, O.svt_oracle_full_distortion32_avx2):
        out = np.zeros(2, np.uint64)
        if eob[0] == 0:
            c2 = int((co.astype(np.int64) ** 2).sum())
            out[:] = c2
        else:
            fn(ptr(co), kw, ptr(dq), kw, ptr(out), kw, kh)
        v = [int(x) + int(en[0]) for x in out]
        res.append([x >> sh if sh >= 0 else (x << -sh) & ((1 << 64) - 1) for x in v])
    return res[0], res[1], int(eob[0]), q, dq


@pytest.mark.parametrize("dense_pred", [False, True])
def test_oracle_at_scale_every_size_all_types(dsp, dense_pred):
    O = svtlibs.oracle()
    rng = np.random.default_rng(13651 + dense_pred)
    qx = 120
    qrow = qrow_of(qx)
    PW, PH = 512, 320
    srcp = rng.integers(0, 256, size=(PH, PW), dtype=np.uint8)
    predp = np.clip(srcp.astype(np.int16) + rng.integers(-20, 21, size=(PH, PW)), 0, 255).astype(np.uint8)
    predp[:, ::7] = rng.integers(0, 256, size=predp[:, ::7].shape, dtype=np.uint8)
    d_src, d_predp = torch.from_numpy(srcp).to(DEV), torch.from_numpy(predp).to(DEV)
    groups, meta = [], []
    for s in range(19):
        w, h = TX_W[s], TX_H[s]
        n = 1024 if max(w, h) <= 16 else 96
        xs = rng.integers(0, PW - w + 1, size=n); ys = rng.integers(0, PH - h + 1, size=n)
        xy = (xs | (ys << 16)).astype(np.int32)
        types = allowed(s)
        rng.shuffle(types)
        sb = np.stack([srcp[y:y + h, x:x + w] for x, y in zip(xs, ys)])
        pb = np.stack([predp[y:y + h, x:x + w] for x, y in zip(xs, ys)])
        g = dict(src=d_src, src_stride=PW, src_xy=torch.from_numpy(xy).to(DEV), nblocks=n, tx_size=s, tx_types=types,
                 iscan=iscans(s, types), **outputs(n, s, len(types)))
        if dense_pred:
            g["pred"] = torch.from_numpy(pb).to(DEV)
        else:
            g.update(pred=d_predp, pred_stride=PW, pred_xy=g["src_xy"])
        groups.append(g); meta.append((s, types, sb, pb))
    run(dsp, groups, qrow, 0)
    dist_c = [g["dist"].cpu().numpy().view(np.uint64) for g in groups]
    run(dsp, groups, qrow, 1)
    for g, dc_all, (s, types, sb, pb) in zip(groups, dist_c, meta):
        da_all, eob = g["dist"].cpu().numpy().view(np.uint64), g["eob"].cpu().numpy().astype(np.int64)
        q, dq = g["qcoeff"].cpu().numpy(), g["dqcoeff"].cpu().numpy()
        for ti, t in enumerate(types):
            isc = svtlibs.scan_tables(s, t)[1]
            for b in range(g["nblocks"]):
                dc, da, e, rq, rdq = oracle_chain(O, s, t, qrow, sb[b], pb[b], isc)
                assert [int(v) for v in dc_all[b, ti]] == dc, (s, t, b)
                assert [int(v) for v in da_all[b, ti]] == da, (s, t, b)
                assert eob[b, ti] == e, (s, t, b)
                assert np.array_equal(q[b, ti], rq) and np.array_equal(dq[b, ti], rdq), (s, t, b)


def test_type_order_multi_type_group_equals_single_type_groups(dsp):
    rng = np.random.default_rng(13652)
    qrow = qrow_of(90)
    for s in (1, 2, 7, 13, 3, 9, 4):
        w, h = TX_W[s], TX_H[s]
        n = 300
        src = torch.from_numpy(rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)).to(DEV)
        pred = torch.from_numpy(np.clip(src.cpu().numpy().astype(np.int16) + rng.integers(-9, 10, size=(n, h, w)), 0, 255).astype(np.uint8)).to(DEV)
        types = allowed(s)[::-1]
        multi = dict(src=src, pred=pred, nblocks=n, tx_size=s, tx_types=types, iscan=iscans(s, types), **outputs(n, s, len(types)))
        singles = [dict(src=src, pred=pred, nblocks=n, tx_size=s, tx_types=[t], iscan=iscans(s, [t]), **outputs(n, s, 1)) for t in types]
        for flavour in (0, 1):
            run(dsp, [multi] + singles, qrow, flavour)
            for ti, g in enumerate(singles):
                for k in ("dist", "eob", "qcoeff", "dqcoeff"):
                    assert torch.equal(multi[k][:, ti], g[k][:, 0]), (s, types[ti], k)
            # the dense convenience call (scans from the package's own tables) gives the same
            dist, eob, q, dq = dsp.full_loop(src, pred, s, types, qrow, flavour, want_qcoeff=True, want_dqcoeff=True)
            torch.cuda.synchronize()
            assert torch.equal(dist, multi["dist"]) and torch.equal(eob, multi["eob"]) and torch.equal(q, multi["qcoeff"]) and torch.equal(dq, multi["dqcoeff"]), s


def test_every_output_written_and_optional_coeffs(dsp):
    rng = np.random.default_rng(13653)
    qrow = qrow_of(200)
    for s in range(19):
        w, h = TX_W[s], TX_H[s]
        n = 77                                     # not a multiple of any workgroup's block count
        src = torch.from_numpy(rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)).to(DEV)
        pred = torch.from_numpy(rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)).to(DEV)
        types = allowed(s)
        a = dict(src=src, pred=pred, nblocks=n, tx_size=s, tx_types=types, iscan=iscans(s, types), **outputs(n, s, len(types)))
        b = dict(src=src, pred=pred, nblocks=n, tx_size=s, tx_types=types, iscan=iscans(s, types), **outputs(n, s, len(types), False))
        run(dsp, [a, b], qrow, 1)
        sent = lambda x: bool((x.view(torch.uint8).view(-1, x.element_size()) == SENT).all(1).any())
        for k in ("dist", "eob", "qcoeff", "dqcoeff"):
            assert not sent(a[k]), (s, k)
        assert torch.equal(a["dist"], b["dist"]) and torch.equal(a["eob"], b["eob"]), s


def test_picture_scale_against_the_composed_library_path(dsp):
    """1080p luma, 6 candidate predictions per 8x8 / 16x16 block and 2 per 32x32 / 64x64 block: the fused call against
    svt_hip_fwd_quant_planes_batch (+ three_quad_energy) -> eob to uint32 -> svt_hip_picture_full_distortion32_batch, per type"""
    g = torch.Generator(device=DEV); g.manual_seed(13654)
    W, H, HP = 1920, 1080, 1088
    src = torch.randint(0, 256, (HP, W), dtype=torch.uint8, device=DEV, generator=g)
    qrow = qrow_of(140)
    tabs = [np.ascontiguousarray(qrow[k]) for k in ("zbin", "round", "quant", "quant_shift", "dequant")]
    for s, ncand in ((1, 6), (2, 6), (3, 2), (4, 2)):
        w, h = TX_W[s], TX_H[s]
        ys, xs = torch.meshgrid(torch.arange(0, H - h + 1, h, device=DEV), torch.arange(0, W - w + 1, w, device=DEV), indexing="ij")
        org = (xs.reshape(-1) | (ys.reshape(-1) << 16)).to(torch.int32)
        nb = org.numel()
        noise = torch.randint(-12, 13, (ncand, HP, W), dtype=torch.int16, device=DEV, generator=g)
        predp = (src.to(torch.int16).unsqueeze(0) + noise * torch.arange(1, ncand + 1, device=DEV).view(-1, 1, 1)).clamp_(0, 255).to(torch.uint8)
        predp = predp.reshape(ncand * HP, W).contiguous()
        src_xy = org.repeat(ncand)                                         # every candidate repeats its block's origin
        pred_xy = (org.view(1, -1) + (torch.arange(ncand, device=DEV, dtype=torch.int32) * HP).view(-1, 1) * 65536).reshape(-1)
        n = nb * ncand
        types = allowed(s) if s <= 2 else allowed(s)[:2]
        for flavour in (0, 1):
            o = outputs(n, s, len(types))
            grp = dict(src=src, src_stride=W, src_xy=src_xy, pred=predp, pred_stride=W, pred_xy=pred_xy, nblocks=n, tx_size=s,
                       tx_types=types, iscan=iscans(s, types), **o)
            run(dsp, [grp], qrow, flavour)
            srcrep = src.repeat(ncand, 1).contiguous()
            for ti, t in enumerate(types):
                isc = iscans(s, [t])[0].contiguous()
                co, q, dq, eob, _, en = dsp.fwd_quant_planes(srcrep, W, predp, W, pred_xy, s, t, qrow, isc, want_energy=True)
                nz = eob.to(torch.int32) & 0xffff
                dist = torch.empty((n, 2), dtype=torch.int64, device=DEV)
                rc = dsp.lib.svt_hip_picture_full_distortion32_batch(dsp._p(co), co.shape[1], dsp._p(dq), dq.shape[1], w, h, dsp._p(nz), flavour,
                                                                     dsp._p(dist), n, dsp._stream())
                assert rc == 0
                pels = w * h
                want = dist + en.view(-1, 1)
                want = want >> 2 if pels <= 256 else (want if pels <= 1024 else want << 2)
                torch.cuda.synchronize()
                assert torch.equal(o["dist"][:, ti], want), (s, t, flavour)
                assert torch.equal(o["eob"][:, ti], eob.view(torch.int16)), (s, t)
                assert torch.equal(o["qcoeff"][:, ti], q) and torch.equal(o["dqcoeff"][:, ti], dq), (s, t)


def test_argument_validation_launches_nothing(dsp):
    s = 1
    n = 64
    src = torch.randint(0, 256, (n, 8, 8), dtype=torch.uint8, device=DEV)
    qrow = qrow_of(100)
    good = lambda **kw: dict(dict(src=src, pred=src, nblocks=n, tx_size=s, tx_types=[0, 1], iscan=iscans(s, [0, 1]), **outputs(n, s, 2)), **kw)
    bad_qs = dict(qrow); bad_qs["quant_shift"] = qrow["quant_shift"].copy(); bad_qs["quant_shift"][1] = 3
    cases = [([good(), dict(nblocks=0, tx_size=200, tx_types=[0])], qrow),                         # empty group, tx_size 200
             ([good(), good(tx_size=3, tx_types=[0, 1], iscan=iscans(3, [0, 0]))], qrow),         # ADST_DCT is not defined for 32x32
             ([good(), good(tx_types=[])], qrow),                                                   # ntypes 0
             ([good(), good(tx_types=list(range(16)), ntypes=17)], qrow),                            # ntypes 17
             ([good(), good(tx_types=[3, 5, 3])], qrow),                                            # duplicate types
             ([good()], bad_qs)]                                                                     # non-power-of-two quant_shift
    for i, (groups, qr) in enumerate(cases):
        first = groups[0]
        rc = dsp.full_loop_frame(groups, qr, 1)
        torch.cuda.synchronize()
        assert rc == -2, (i, rc)
        assert bool((first["dist"].view(torch.uint8) == SENT).all()) and bool((first["eob"].view(torch.uint8) == SENT).all()), i
    assert dsp.full_loop_frame([good()], qrow, 2) == -2                                              # flavour


def test_more_groups_of_one_class_than_one_launch_holds(dsp):
    """17 groups of 8x8 blocks, one transform type: one more than a launch's table holds (FL_MAX_GROUPS = 16), so the call takes a
    second launch whose table starts again from its group's own workgroup count.  Sixteen groups of 5 blocks and one of 40 (two
    workgroups of 32 blocks), distinct data per group; both distortion flavours and the eob against the CPU oracle."""
    O = svtlibs.oracle()
    rng = np.random.default_rng(13655)
    s, t = 1, 0
    qrow = qrow_of(110)
    isc = svtlibs.scan_tables(s, t)[1]
    groups, data = [], []
    for gi in range(17):
        n = 40 if gi == 3 else 5
        sb = rng.integers(0, 256, size=(n, 8, 8), dtype=np.uint8)
        pb = np.clip(sb.astype(np.int16) + rng.integers(-30, 31, size=(n, 8, 8)), 0, 255).astype(np.uint8)
        groups.append(dict(src=torch.from_numpy(sb).to(DEV), pred=torch.from_numpy(pb).to(DEV), nblocks=n, tx_size=s, tx_types=[t],
                           iscan=iscans(s, [t]), **outputs(n, s, 1, False)))
        data.append((sb, pb))
    run(dsp, groups, qrow, 0)
    dist_c = [g["dist"].cpu().numpy().view(np.uint64).copy() for g in groups]
    eob_c = [g["eob"].cpu().numpy().copy() for g in groups]
    run(dsp, groups, qrow, 1)
    for gi, (g, (sb, pb)) in enumerate(zip(groups, data)):
        da_all, eob = g["dist"].cpu().numpy().view(np.uint64), g["eob"].cpu().numpy()
        for b in range(g["nblocks"]):
            dc, da, e, _, _ = oracle_chain(O, s, t, qrow, sb[b], pb[b], isc)
            assert [int(v) for v in dist_c[gi][b, 0]] == dc, (gi, b)
            assert [int(v) for v in da_all[b, 0]] == da, (gi, b)
            assert int(eob_c[gi][b, 0]) == e and int(eob[b, 0]) == e, (gi, b)
