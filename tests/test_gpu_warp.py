"""GPU: svt_hip_warp_fit_frame and svt_hip_warp_pred_frame against tests/golden/warp.npz (the compiled reference's warped_filter,
find_projection and av1_warp_plane[_hbd] behind tests/c/ref_warp.c, see tests/golden/make_golden_warp.py) and, where a test composes
calls, against the restatements of tests/warp_cases.py and tests/golden/make_golden_inter_fast.py composed the same way.  Every output
is allocated poisoned and fenced (tests/poison.py); every comparison is an equality."""
import os
import sys

import numpy as np
import pytest
import torch

import layouts
import poison
import warp_cases as wc
from poison import poisoned_outputs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

pytestmark = pytest.mark.gpu
SAD, SSD = 0, 1
PLANES = ("y", "cb", "cr")
_gold = None
_dev = {}


def gold():
    global _gold
    if _gold is None:
        _gold = dict(np.load(wc.FIXTURE))
    return _gold


def up(dsp, a):
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    if a.dtype in (np.uint64, np.uint32, np.uint16):
        a = a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}[a.dtype])
    return torch.from_numpy(a).to(dsp.device)


def ok(dsp, rc):
    assert rc == 0, dsp.lib.svt_hip_last_error().decode()
    torch.cuda.synchronize()


def tdtype(bd):
    return torch.uint8 if bd == 8 else torch.int16


def to_np(t, bd):
    a = t.cpu().numpy()
    return a if bd == 8 else a.view(np.uint16)


def fill_of(bd):
    return poison.fill_value(tdtype(bd)) & ((1 << 16) - 1 if bd > 8 else 0xff)


def picture(dsp, pi):
    """(w, h, bd, numpy planes, device planes), uploaded once and never written"""
    if ("pic", pi) not in _dev:
        g = gold()
        w, h, bd = (int(v) for v in g["pictures"][pi])
        planes = [g[f"pic{pi}_{n}"] for n in PLANES]
        _dev[("pic", pi)] = (w, h, bd, planes, [up(dsp, p) for p in planes])
    return _dev[("pic", pi)]


def source(pi, pl):
    """a source plane for the fused distortion: noise of the picture's depth"""
    g = gold()
    w, h, bd = (int(v) for v in g["pictures"][pi])
    rng = np.random.default_rng([0x57A, pi, pl])
    return rng.integers(0, 1 << bd, (h >> (pl > 0), w >> (pl > 0))).astype(np.uint8 if bd == 8 else np.uint16)


def cases_of(pi):
    """the fixture's prediction cases of a picture, grouped by (plane, luma bw, luma bh): {key: [(x, y, model row, expected block)]}"""
    g = gold()
    bd = int(g["pictures"][pi][2])
    data = g[f"pred_data_{bd}"]
    groups = {}
    for c in g["pred_cases"]:
        p, pl, bw, bh, x, y, mi, off = (int(v) for v in c)
        if p != pi:
            continue
        ss = int(pl > 0)
        pw, ph = bw >> ss, bh >> ss
        groups.setdefault((pl, bw, bh), []).append((x, y, g["pred_models"][mi], data[off:off + pw * ph].reshape(ph, pw)))
    return groups


def records(pkg, cases, invalid_last=True):
    """blk and model records [n + 1][1] of a case list; the last record (a copy of the first) has valid 0"""
    n = len(cases) + int(invalid_last)
    blk, model = np.zeros((n, 1), pkg.inter_blk_dtype()), np.zeros((n, 1), pkg.warp_model_dtype())
    for i in range(n):
        x, y, m, _ = cases[i % len(cases)]
        blk[i, 0]["x"], blk[i, 0]["y"] = x, y
        model[i, 0]["mat"], model[i, 0]["valid"] = m[:6], int(i < len(cases))
        for k, name in enumerate(("alpha", "beta", "gamma", "delta")):
            model[i, 0][name] = m[6 + k]
    return blk, model


def non_overlapping(cases, bw, bh):
    out = []
    for c in cases:
        if all(abs(c[0] - o[0]) >= bw or abs(c[1] - o[1]) >= bh for o in out):
            out.append(c)
    return out


# ---- the fit -----------------------------------------------------------------------------------------------------------------------------
def fit_inputs(pkg, ncand):
    """the fixture's records, one group per block size: candidate 0 is the recorded vector, the others lie round it"""
    g = gold()
    rng = np.random.default_rng(0xF17)
    groups = []
    for bsize in sorted(set(int(b) for b in g["fit_bsize"])):
        idx = np.nonzero(g["fit_bsize"] == bsize)[0]
        samples = np.zeros(len(idx), pkg.warp_samples_dtype())
        blk = np.zeros((len(idx), ncand), pkg.inter_blk_dtype())
        samples["nsamples"], samples["pts"], samples["pts_inref"] = g["fit_nsamples"][idx], g["fit_pts"][idx], g["fit_pts_inref"][idx]
        blk["x"], blk["y"] = g["fit_xy"][idx, 0:1], g["fit_xy"][idx, 1:2]
        blk["mv"][:, :, 0, :] = g["fit_mv"][idx][:, None, :]
        if ncand > 1:
            blk["mv"][:, 1:, 0, :] += rng.integers(-60, 61, (len(idx), ncand - 1, 2)).astype(np.int16)
        blk["mv"][:, :, 1, :] = 0x1234                      # list 1 is not read
        groups.append((bsize, idx, samples, blk))
    return groups


@pytest.mark.parametrize("ncand", [1, 13])
def test_fit_every_fixture_record_one_group_per_block_size(dsp, pkg, ncand):
    g = gold()
    inputs = fit_inputs(pkg, ncand)
    assert {b for b, _, _, _ in inputs} == set(wc.WARP_BSIZES), "one group per block-size class"
    dev = []
    for bsize, idx, samples, blk in inputs:
        dev.append(dict(bsize=bsize, ncand=ncand, samples=up(dsp, samples), blk=up(dsp, blk),
                        model=poison.tensor((len(idx), ncand, 36), torch.uint8, dsp.device), nvalid=poison.tensor((len(idx),), torch.int32, dsp.device)))
    ok(dsp, dsp.warp_fit_frame(dev))
    for (bsize, idx, samples, blk), d in zip(inputs, dev):
        got = d["model"].cpu().numpy().view(pkg.warp_model_dtype())[..., 0]
        want, nvalid = wc.fit_group(samples, blk, bsize)
        for k in wc.MODEL_FIELDS:
            bad = np.argwhere(got[k] != want[k])
            assert bad.size == 0, (bsize, k, bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
        assert not got["pad"].any()
        assert np.array_equal(d["nvalid"].cpu().numpy().view(np.uint32), nvalid), bsize
        # candidate 0 against the reference's own record
        ref = g["fit_ref"][idx]
        assert np.array_equal(got["num_proj_ref"][:, 0], ref[:, 0]) and np.array_equal(got["valid"][:, 0] == 1, ref[:, 1] == 0)
        assert np.array_equal(got["mat"][:, 0], ref[:, 2:8])
        assert np.array_equal(np.stack([got[k][:, 0] for k in ("alpha", "beta", "gamma", "delta")], axis=1), ref[:, 8:12])


# ---- the prediction, direct mode ---------------------------------------------------------------------------------------------------------
def direct_groups(dsp, pkg, pi, mode, metric=SAD):
    """every (plane, shape) group of a picture's fixture cases with poisoned outputs -> (groups, checks)"""
    w, h, bd, planes_np, planes = picture(dsp, pi)
    groups, checks = [], []
    for (pl, bw, bh), cases in sorted(cases_of(pi).items()):
        ss = int(pl > 0)
        pw, ph = bw >> ss, bh >> ss
        if mode == "strided":
            cases = non_overlapping(cases, bw, bh)
        blk, model = records(pkg, cases)
        n = len(blk)
        d = dict(ref=planes[pl], ref_stride=planes_np[pl].shape[1], ss=ss, bwidth=bw, bheight=bh, ncand=1, blk=up(dsp, blk), model=up(dsp, model))
        if mode == "dense":
            d["pred"] = poison.tensor((n, ph, pw), tdtype(bd), dsp.device)
        elif mode == "strided":
            d["pred_stride"] = (w >> ss) + 5
            d["pred"] = poison.tensor((h >> ss, d["pred_stride"]), tdtype(bd), dsp.device)
        else:
            src = source(pi, pl)
            d.update(src=up(dsp, src), src_stride=src.shape[1], dist=poison.tensor((n,), torch.int64, dsp.device))
        groups.append(d)
        checks.append((pl, bw, bh, cases))
    return groups, checks


@pytest.mark.parametrize("pi", [0, 1, 2, 3])
@pytest.mark.parametrize("mode", ["dense", "strided", "sad", "ssd"])
def test_direct_mode_every_fixture_case(dsp, pkg, pi, mode):
    """every shape, luma and chroma, corners and edges, every model of the fixture; the record with valid 0 leaves the poison"""
    w, h, bd, _, _ = picture(dsp, pi)
    metric = SSD if mode == "ssd" else SAD
    groups, checks = direct_groups(dsp, pkg, pi, mode, metric)
    shapes = {(bw, bh) for _, bw, bh, _ in checks}
    assert shapes == {(8, 8), (16, 8), (8, 16), (16, 16), (32, 16), (64, 32), (64, 64)}
    ok(dsp, dsp.warp_pred_frame(groups, w, h, bd, metric))
    fill = fill_of(bd)
    for d, (pl, bw, bh, cases) in zip(groups, checks):
        ss = int(pl > 0)
        if mode == "dense":
            got = to_np(d["pred"], bd)
            for i, c in enumerate(cases):
                assert np.array_equal(got[i], c[3]), (pl, bw, bh, i, c[0], c[1])
            assert (got[len(cases)] == fill).all(), "the invalid model's slot"
        elif mode == "strided":
            want = np.full((h >> ss, d["pred_stride"]), fill, np.uint8 if bd == 8 else np.uint16)
            for c in cases:
                want[c[1] >> ss:(c[1] + bh) >> ss, c[0] >> ss:(c[0] + bw) >> ss] = c[3]
            assert np.array_equal(to_np(d["pred"], bd), want), (pl, bw, bh)
        else:
            src = source(pi, pl)
            got = d["dist"].cpu().numpy()
            for i, c in enumerate(cases):
                s = src[c[1] >> ss:(c[1] + bh) >> ss, c[0] >> ss:(c[0] + bw) >> ss]
                assert int(got[i]) == wc.distortion(c[3], s, metric), (pl, bw, bh, i)
            assert int(got[len(cases)]) == poison.fill_value(torch.int64), "the invalid model's slot"


def test_prediction_and_distortion_in_one_call_more_groups_than_one_launch(dsp, pkg):
    """d_pred and d_dist together; 50 non-empty groups and two empty ones: two launches"""
    pi = 0
    w, h, bd, planes_np, planes = picture(dsp, pi)
    all_cases = cases_of(pi)
    keys = sorted(all_cases)
    groups, checks = [], []
    for k in range(52):
        pl, bw, bh = keys[k % len(keys)]
        ss = int(pl > 0)
        cases = all_cases[(pl, bw, bh)][k % 3::3][:4] if k not in (7, 30) else []
        blk, model = records(pkg, cases or all_cases[(pl, bw, bh)][:1], invalid_last=False)
        src = source(pi, pl)
        n = len(cases)
        groups.append(dict(ref=planes[pl], ref_stride=planes_np[pl].shape[1], ss=ss, bwidth=bw, bheight=bh, ncand=1, nblocks=n, blk=up(dsp, blk),
                           model=up(dsp, model), pred=poison.tensor((max(n, 1), bh >> ss, bw >> ss), torch.uint8, dsp.device), src=up(dsp, src),
                           src_stride=src.shape[1], dist=poison.tensor((max(n, 1),), torch.int64, dsp.device)))
        checks.append((pl, bw, bh, cases, src))
    ok(dsp, dsp.warp_pred_frame(groups, w, h, bd, SSD))
    for d, (pl, bw, bh, cases, src) in zip(groups, checks):
        ss = int(pl > 0)
        got, dist = d["pred"].cpu().numpy(), d["dist"].cpu().numpy()
        for i, c in enumerate(cases):
            assert np.array_equal(got[i], c[3])
            assert int(dist[i]) == wc.distortion(c[3], src[c[1] >> ss:(c[1] + bh) >> ss, c[0] >> ss:(c[0] + bw) >> ss], SSD)
        if not cases:
            assert (got == fill_of(8)).all() and int(dist[0]) == poison.fill_value(torch.int64)


# ---- the prediction, survivors mode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi,pl,bw,bh", [(0, 0, 16, 16), (2, 1, 32, 16), (3, 0, 64, 32)])
def test_survivors_mode_entries_below_inside_and_above_the_range(dsp, pkg, pi, pl, bw, bh):
    w, h, bd, planes_np, planes = picture(dsp, pi)
    cases = cases_of(pi)[(pl, bw, bh)]
    ss = int(pl > 0)
    ncand, n, first = 4, 5, 3
    nb = len(cases) // ncand
    blk1, model1 = records(pkg, cases[:nb * ncand], invalid_last=False)
    blk, model = blk1.reshape(nb, ncand), model1.reshape(nb, ncand).copy()
    model["valid"][1::3, 2] = 0                                       # some selected records have no model
    rng = np.random.default_rng(0x5E1)
    sel = rng.integers(0, first + ncand + 3, (nb, n)).astype(np.uint8)
    sel[0] = (first - 1, first, first + ncand - 1, first + ncand, 255)
    assert (sel < first).any() and (sel >= first + ncand).any() and ((sel >= first) & (sel < first + ncand)).any()
    src = source(pi, pl)
    d = dict(ref=planes[pl], ref_stride=planes_np[pl].shape[1], ss=ss, bwidth=bw, bheight=bh, ncand=ncand, blk=up(dsp, blk), model=up(dsp, model),
             sel=up(dsp, sel), sel_first=first, pred=poison.tensor((nb, n, bh >> ss, bw >> ss), tdtype(bd), dsp.device), src=up(dsp, src),
             src_stride=src.shape[1], dist=poison.tensor((nb, n), torch.int64, dsp.device))
    ok(dsp, dsp.warp_pred_frame([d], w, h, bd, SAD))
    got, dist = to_np(d["pred"], bd), d["dist"].cpu().numpy()
    written = 0
    for b in range(nb):
        for s in range(n):
            c = int(sel[b, s]) - first
            if 0 <= c < ncand and model[b, c]["valid"]:
                x, y, _, want = cases[b * ncand + c]
                assert np.array_equal(got[b, s], want), (b, s, c)
                assert int(dist[b, s]) == wc.distortion(want, src[y >> ss:(y + bh) >> ss, x >> ss:(x + bw) >> ss], SAD)
                written += 1
            else:
                assert (got[b, s] == fill_of(bd)).all() and int(dist[b, s]) == poison.fill_value(torch.int64), (b, s, c)
    assert 0 < written < nb * n


# ---- one layout test: no two of the ref / pred / src strides, origins and pitches are equal -------------------------------------------------
def test_ref_pred_and_src_each_at_a_layout_of_its_own(dsp, pkg, request):
    pi, pl, bw, bh = 0, 0, 16, 16
    w, h, bd, planes_np, _ = picture(dsp, pi)
    fill = getattr(request.function, "poison_fill", poison.FILLS[0])
    spec = layouts.CallSpec("svt_hip_warp_pred_frame", [layouts.Plane(n, w, h, stacked=False) for n in ("ref", "pred", "src")])
    lay = layouts.distinct_layouts(spec)
    cases = non_overlapping(cases_of(pi)[(pl, bw, bh)], bw, bh)
    blk, model = records(pkg, cases)
    src = source(pi, pl)
    placed = {}
    for name, content in (("ref", planes_np[pl]), ("pred", layouts.poison_like(planes_np[pl], fill)), ("src", src)):
        placed[name] = layouts.place_plane(spec.plane(name), content, lay[name], fill=fill) + (content,)
    d = dict(ref=placed["ref"][1], ref_stride=lay["ref"].stride, ss=0, bwidth=bw, bheight=bh, ncand=1, blk=up(dsp, blk), model=up(dsp, model),
             pred=placed["pred"][1], pred_stride=lay["pred"].stride, src=placed["src"][1], src_stride=lay["src"].stride,
             dist=poison.tensor((len(blk),), torch.int64, dsp.device))
    ok(dsp, dsp.warp_pred_frame([d], w, h, bd, SSD))
    want = layouts.poison_like(planes_np[pl], fill)
    dist = d["dist"].cpu().numpy()
    for i, (x, y, _, blkpred) in enumerate(cases):
        want[y:y + bh, x:x + bw] = blkpred
        assert int(dist[i]) == wc.distortion(blkpred, src[y:y + bh, x:x + bw], SSD)
    assert np.array_equal(placed["pred"][1].cpu().numpy(), want)
    for name in ("ref", "src"):
        layouts.assert_guards_intact(placed[name][0], placed[name][1], fill, name, placed[name][2])
    layouts.assert_guards_intact(placed["pred"][0], placed["pred"][1], fill, "pred")


# ---- the chain: fit, direct distortion on Y / Cb / Cr, the existing pick, survivors mode -------------------------------------------------------
def chain_inputs(pkg):
    import make_golden_inter_fast as mg
    rng = np.random.default_rng(0xC4A1)
    nb, ni, bsize = 6, 13, 6                                           # 16x16
    xy = [(16, 0), (48, 16), (0, 32), (80, 48), (32, 56), (88, 0)]
    samples = np.zeros(nb, pkg.warp_samples_dtype())
    blk, cand = mg.make_candidates(rng, nb, ni, xy, search=True)
    for b in range(nb):
        while True:
            d = wc.draw_fit(rng, bsize=bsize, kind=1 + b % 2)
            if d["nsamples"] >= 3:
                break
        mv = rng.integers(-24, 25, 2)
        samples[b]["nsamples"], samples[b]["pts"] = d["nsamples"], d["pts"]
        samples[b]["pts_inref"] = d["pts"] + np.tile(mv, 8) + rng.integers(-3, 4, 16)
        blk[b]["mv"][:, 0, :] = mv + rng.integers(-6, 7, (ni, 2))
        blk[b]["mv"][:, 1, :] = 0
    blk[2, 12]["mv"][0] = (3000, -3000)                                # no sample near it: the one kept sample fails LS_MV_MAX, no model
    blk["pred_direction"] = 0
    cand["pred_mode"], cand["ref_frame_type"] = mg.NEWMV, mg.LAST
    cand["flags"] = (cand["flags"] & 1) | 2 << 1 | 2 << 3              # motion_mode WARPED_CAUSAL, allowed
    ctx = mg.make_ctx(rng, nb)
    P = dict(ninter=ni, nintra=0, nfl=3, bsize=bsize, bsize_uv=3, metric=mg.SAD, ac_dequant_q3=0, reference_mode_select=1, switchable_motion_mode=1,
             chroma=1, intra_rate=0, rate_set=1)
    P["lambda"] = 29041
    return mg, P, samples, blk, cand, ctx


def test_chain_fit_distortion_pick_and_survivors(dsp, pkg):
    """16x16, 6 blocks, 13 warped candidates per block, nfl 3, 4:2:0: the four calls on the device against the restatements composed
    the same way.  A candidate without a model keeps the distortion its slot was given (NO_MODEL), as a caller would arrange it."""
    mg, P, samples, blk, cand, ctx = chain_inputs(pkg)
    pi, bw, bh, NO_MODEL = 0, 16, 16, 1 << 28
    w, h, bd, planes_np, planes = picture(dsp, pi)
    nb, ni, n = len(samples), P["ninter"], P["nfl"]
    table = gold()["table"]
    # ---- the restatements ----
    model, nvalid = wc.fit_group(samples, blk, P["bsize"])
    assert 0 < (model["valid"] == 0).sum() < nb * ni and model["valid"][2, 12] == 0
    srcs = [source(pi, pl) for pl in range(3)]
    preds = [np.zeros((nb, ni, bh >> (pl > 0), bw >> (pl > 0)), np.uint8) for pl in range(3)]
    dist = [np.full((nb, ni), NO_MODEL, np.int64) for _ in range(3)]
    for b in range(nb):
        for c in range(ni):
            if not model["valid"][b, c]:
                continue
            x, y = int(blk[b, c]["x"]), int(blk[b, c]["y"])
            shear = [model[k][b, c] for k in ("alpha", "beta", "gamma", "delta")]
            for pl in range(3):
                ss = int(pl > 0)
                preds[pl][b, c] = wc.warp_pred(table, planes_np[pl], bd, x >> ss, y >> ss, bw >> ss, bh >> ss, ss, model["mat"][b, c], shear)
                dist[pl][b, c] = wc.distortion(preds[pl][b, c], srcs[pl][y >> ss:(y + bh) >> ss, x >> ss:(x + bw) >> ss], SAD)
    R = mg.make_rates(P["rate_set"])
    mv_cost = mg.make_mv_cost()
    want = mg.pick_group(P, R, mv_cost, blk, cand, ctx, dist[0], dist[1], dist[2], None, None)
    # ---- the device ----
    d_blk, d_model = up(dsp, blk), poison.tensor((nb, ni, 36), torch.uint8, dsp.device)
    ok(dsp, dsp.warp_fit_frame([dict(bsize=P["bsize"], ncand=ni, samples=up(dsp, samples), blk=d_blk, model=d_model)]))
    d_dist = [poison.tensor((nb, ni), torch.int64, dsp.device) for _ in range(3)]
    for t in d_dist:
        t.fill_(NO_MODEL)
    common = dict(bwidth=bw, bheight=bh, ncand=ni, blk=d_blk, model=d_model)
    d_src = [up(dsp, s) for s in srcs]
    ok(dsp, dsp.warp_pred_frame([dict(common, ref=planes[pl], ref_stride=planes_np[pl].shape[1], ss=int(pl > 0), src=d_src[pl],
                                      src_stride=srcs[pl].shape[1], dist=d_dist[pl]) for pl in range(3)], w, h, bd, SAD))
    for pl in range(3):
        assert np.array_equal(d_dist[pl].cpu().numpy(), dist[pl]), pl
    pick = dict(bsize=P["bsize"], bsize_uv=P["bsize_uv"], nblocks=nb, ninter=ni, nintra=0, nfl=n, ac_dequant_q3=0, reference_mode_select=1,
                switchable_motion_mode=1, blk=d_blk, cand_in=up(dsp, cand), ctx=up(dsp, ctx), rates=up(dsp, mg.pack_rates(R)), mv_cost=up(dsp, mv_cost),
                dist=d_dist[0], dist_cb=d_dist[1], dist_cr=d_dist[2], cand=poison.tensor((nb, n), torch.uint8, dsp.device),
                sorted=poison.tensor((nb, n), torch.uint8, dsp.device), cost=poison.tensor((nb, n), torch.int64, dsp.device),
                rate=poison.tensor((nb, n, 2), torch.int32, dsp.device), ref_fast_cost=poison.tensor((nb,), torch.int64, dsp.device),
                blk_out=poison.tensor((nb, n, 16), torch.uint8, dsp.device))
    pick["lambda"] = P["lambda"]
    ok(dsp, dsp.inter_fast_pick_frame([pick], SAD))
    assert np.array_equal(pick["cand"].cpu().numpy(), want["cand"]) and np.array_equal(pick["cost"].cpu().numpy().view(np.uint64), want["cost"])
    d_pred = [poison.tensor((nb, n, bh >> (pl > 0), bw >> (pl > 0)), torch.uint8, dsp.device) for pl in range(3)]
    ok(dsp, dsp.warp_pred_frame([dict(common, ref=planes[pl], ref_stride=planes_np[pl].shape[1], ss=int(pl > 0), sel=pick["cand"], sel_first=0,
                                      pred=d_pred[pl]) for pl in range(3)], w, h, bd, SAD))
    for pl in range(3):
        got = d_pred[pl].cpu().numpy()
        for b in range(nb):
            for s in range(n):
                c = int(want["cand"][b, s])
                if model["valid"][b, c]:
                    assert np.array_equal(got[b, s], preds[pl][b, c]), (pl, b, s, c)
                else:
                    assert (got[b, s] == fill_of(8)).all(), (pl, b, s, c)


# ---- graph capture: fit -> prediction, replayed once --------------------------------------------------------------------------------------
def test_fit_then_prediction_captured_in_a_graph_and_replayed(dsp, pkg):
    mg, P, samples, blk, cand, ctx = chain_inputs(pkg)
    pi, bw, bh = 0, 16, 16
    w, h, bd, planes_np, planes = picture(dsp, pi)
    nb, ni = len(samples), P["ninter"]
    model, _ = wc.fit_group(samples, blk, P["bsize"])
    table = gold()["table"]
    src = source(pi, 0)
    d_samples, d_blk, d_src = up(dsp, samples), up(dsp, blk), up(dsp, src)
    d_model = poison.tensor((nb, ni, 36), torch.uint8, dsp.device)
    d_pred = poison.tensor((nb, ni, bh, bw), torch.uint8, dsp.device)
    d_dist = poison.tensor((nb, ni), torch.int64, dsp.device)
    fit = dsp.make_warp_fit_groups([dict(bsize=P["bsize"], ncand=ni, samples=d_samples, blk=d_blk, model=d_model)])
    pred = dsp.make_warp_pred_groups([dict(ref=planes[0], ref_stride=w, ss=0, bwidth=bw, bheight=bh, ncand=ni, blk=d_blk, model=d_model, pred=d_pred,
                                           src=d_src, src_stride=w, dist=d_dist)])
    stream = torch.cuda.Stream(device=dsp.device)
    stream.wait_stream(torch.cuda.current_stream(dsp.device))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            rc = (dsp.warp_fit_frame(fit), dsp.warp_pred_frame(pred, w, h, bd, SAD))
    torch.cuda.current_stream(dsp.device).wait_stream(stream)
    assert rc == (0, 0), dsp.lib.svt_hip_last_error().decode()
    torch.cuda.synchronize()
    assert (d_model == poison.fill_value(torch.uint8)).all(), "capture runs nothing"
    graph.replay()
    torch.cuda.synchronize()
    got_model = d_model.cpu().numpy().view(pkg.warp_model_dtype())[..., 0]
    for k in wc.MODEL_FIELDS:
        assert np.array_equal(got_model[k], model[k]), k
    got, dist = d_pred.cpu().numpy(), d_dist.cpu().numpy()
    for b in range(nb):
        for c in range(ni):
            if model["valid"][b, c]:
                x, y = int(blk[b, c]["x"]), int(blk[b, c]["y"])
                want = wc.warp_pred(table, planes_np[0], bd, x, y, bw, bh, 0, model["mat"][b, c], [model[k][b, c] for k in ("alpha", "beta", "gamma", "delta")])
                assert np.array_equal(got[b, c], want), (b, c)
                assert int(dist[b, c]) == wc.distortion(want, src[y:y + bh, x:x + bw], SAD)
            else:
                assert (got[b, c] == fill_of(8)).all() and int(dist[b, c]) == poison.fill_value(torch.int64)


def test_refusals_return_invalid_and_launch_nothing(dsp, pkg):
    """a few refusals through the library itself (tests/c/warp_plan_host.cpp has every clause): the poisoned outputs stay untouched"""
    w, h, bd, planes_np, planes = picture(dsp, 0)
    cases = cases_of(0)[(0, 16, 16)][:2]
    blk, model = records(pkg, cases, invalid_last=False)
    pred = poison.tensor((2, 16, 16), torch.uint8, dsp.device)
    good = dict(ref=planes[0], ref_stride=w, ss=0, bwidth=16, bheight=16, ncand=1, blk=up(dsp, blk), model=up(dsp, model), pred=pred)
    for edit in (dict(bwidth=4), dict(ss=1, bwidth=8), dict(ncand=0), dict(ncand=65), dict(pred=None), dict(n=2), dict(sel_first=1), dict(ref=None)):
        assert dsp.warp_pred_frame([dict(good, **edit)], w, h, bd, SAD) == -2, edit
    assert dsp.warp_pred_frame([good], w, h, 12, SAD) == -2 and dsp.warp_pred_frame([good], w, h, bd, 2) == -2 and dsp.warp_pred_frame([good], w + 4, h, bd, SAD) == -2
    samples = np.zeros(2, pkg.warp_samples_dtype())
    mdl = poison.tensor((2, 1, 36), torch.uint8, dsp.device)
    fit = dict(bsize=6, ncand=1, samples=up(dsp, samples), blk=up(dsp, blk), model=mdl)
    for edit in (dict(bsize=0), dict(bsize=13), dict(bsize=22), dict(bsize=16), dict(ncand=0), dict(ncand=65), dict(samples=None, nblocks=2), dict(model=None)):
        assert dsp.warp_fit_frame([dict(fit, **edit)]) == -2, edit
    torch.cuda.synchronize()
    assert (pred == poison.fill_value(torch.uint8)).all() and (mdl == poison.fill_value(torch.uint8)).all()


poison.add_second_fill(globals())
