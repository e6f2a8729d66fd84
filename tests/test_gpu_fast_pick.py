"""GPU: svt_hip_fast_pick_frame (fast cost, the N best, their order and the survivors' predictions per block) against the fixture
(tests/golden/fast_pick.npz: the reference's loops restated; on the CPU every cost and rate of it is pinned to the compiled
av1_intra_fast_cost, the SSD model to model_rd_from_sse, the order to sort_fast_loop_candidates, has_chroma to is_chroma_reference) and
its numpy restatement, and svt_hip_intra_fast_search_frame (fast loop -> pick in one call) against what the reference's own
inject_intra_candidates -> perform_fast_loop -> sort_fast_loop_candidates produced on whole blocks (tests/golden/fast_search_ref.npz, no
restatement in between), against the calls enqueued by hand, and as the stage in front of svt_hip_tx_search_frame.  Still the caller's,
and restated nowhere here: inter candidates, the first (src-to-src) loop and the intrabc branch.  Every output is compared for equality
in a poisoned, fenced buffer."""
import os
import sys

import numpy as np
import pytest
import torch

import poison
import svtlibs
from poison import poisoned_outputs  # noqa: F401
from svtlibs import TX_H, TX_W, txfm_allowed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "fast_pick.npz")
FAST_LOOP = os.path.join(ROOT, "tests", "golden", "fast_loop.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_coeff_rate as mgc  # noqa: E402
import make_golden_fast_pick as mg  # noqa: E402
import make_golden_fast_search_ref as ms  # noqa: E402

INVALID = -2
PITCH = 1 + 2 * 64 + 15                                                     # fast_loop.npz keeps 15 samples in front of the corner
SAD, SSD = mg.SAD, mg.SSD
OUT_DTYPES = dict(cand=torch.uint8, sorted=torch.uint8, cost=torch.int64, rate=torch.int32, ref_fast_cost=torch.int64, all_cost=torch.int64,
                  pred_out=torch.uint8, src_xy_out=torch.int32)
NP_VIEW = dict(cost=np.uint64, ref_fast_cost=np.uint64, all_cost=np.uint64, rate=np.uint32, src_xy_out=np.uint32)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint64, np.uint32, np.uint16):                          # torch has the signed types
        a = a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}[a.dtype])
    return torch.from_numpy(a).to(DEV)


def pred_array(n, C, h, w, salt):
    """uint8 [n, C, h, w], a function of the indices with values below 64: neither fill byte can stand in for a sample"""
    i = lambda k, shape: np.arange(k, dtype=np.int64).reshape(shape)
    return ((i(n, (n, 1, 1, 1)) * 29 + i(C, (1, C, 1, 1)) * 7 + i(h, (1, 1, h, 1)) * 3 + i(w, (1, 1, 1, w)) + salt) % 61).astype(np.uint8)


def pick_group(P, dist, cb, cr, blk, rates, gather=True, all_cost=True, salt=0):
    """(group dict with poisoned outputs, expected dict) for the parameters and inputs given; expected from the numpy restatement"""
    n, C = dist.shape
    N = min(P["nfl"], C)
    w, h = TX_W[P["tx_size"]], TX_H[P["tx_size"]]
    g = dict(tx_size=P["tx_size"], bsize=P["bsize"], bsize_uv=P["bsize_uv"], nblocks=n, modes=[int(v) for v in P["modes"]], deltas=[int(v) for v in P["deltas"]],
             uv_modes=[int(v) for v in P["uv_modes"]], uv_deltas=[int(v) for v in P["uv_deltas"]], use_angle_delta=P["use_angle_delta"], nfl=P["nfl"],
             slice_is_intra=P["slice_is_intra"], ac_dequant_q3=P["ac_dequant_q3"], intrabc_bits=P["intrabc_bits"], dist=dev(dist),
             dist_cb=dev(cb) if cb is not None else None, dist_cr=dev(cr) if cr is not None else None, blk=dev(blk.view(np.uint8).reshape(-1, 8)),
             rates=dev(np.asarray(rates, np.int32)), metric=P["metric"])
    g["lambda"] = P["lambda"]
    want = mg.np_fast_pick(P, dist, cb, cr, blk, rates)
    shapes = dict(cand=(n, N), sorted=(n, N), cost=(n, N), rate=(n, N, 2), ref_fast_cost=(n,))
    if all_cost:
        shapes["all_cost"] = (n, C)
    else:
        del want["all_cost"]
    if gather:
        pred = pred_array(n, C, h, w, salt)
        xy = ((np.arange(n, dtype=np.uint32) * 8 + 1) | (np.arange(n, dtype=np.uint32) * 3 + 2) << 16).astype(np.uint32)
        g["pred"], g["src_xy"] = dev(pred), dev(xy)
        shapes["pred_out"], shapes["src_xy_out"] = (n, N, h, w), (n, N)
        want["pred_out"], want["src_xy_out"] = mg.np_gather(want["cand"], pred), np.repeat(xy[:, None], N, axis=1)
    for k, shp in shapes.items():
        g[k] = poison.tensor(shp, OUT_DTYPES[k], DEV)
    return g, want


def case_group(z, ci, **kw):
    P, dist, cb, cr, blk, rates, want_fix = mg.case_of(z, ci)
    g, want = pick_group(P, dist, cb, cr, blk, rates, salt=ci, **kw)
    for k, v in want_fix.items():                                               # the restatement agrees with the stored loops' results
        if k in want:
            assert np.array_equal(want[k], v), (ci, k)
    return g, want


def run(dsp, groups, metric):
    rc = dsp.fast_pick_frame(groups, metric)
    torch.cuda.synchronize()
    assert rc == 0, dsp.lib.svt_hip_last_error()


def check(groups, wants):
    for g, w in zip(groups, wants):
        for k, v in w.items():
            got = g[k].cpu().numpy()
            if k in NP_VIEW:
                got = got.view(NP_VIEW[k])
            bad = np.argwhere(got != v)
            assert bad.size == 0, (g["tx_size"], g["nfl"], k, bad[:6].tolist(), got[tuple(bad[0])], v[tuple(bad[0])])


def by_metric(z):
    out = {SAD: [], SSD: []}
    for ci in range(mg.NCASES):
        out[int(mg.case_of(z, ci)[0]["metric"])].append(ci)
    return out


@pytest.mark.parametrize("metric", [SAD, SSD])
def test_golden_fixture_all_cases_in_one_call(dsp, gold, metric):
    """every fixture case of the metric as the groups of one call, every output asked for: 4x4 (13 candidates, a one-vector gather), 8x8
    (61), 4x16, 16x4, 32x32, 64x64 (the largest gather); nfl 1 (two buffers), 3, 12, 13 = ncand (no scratch), 40 on 61 (41 buffers), 40 on
    13 (clamped); I and non-I slices, with and without chroma distortions, has_chroma mixed, intrabc bits, UV_CFL_PRED, directional uv
    modes with deltas, all-zero tables with three-valued distortions (ties), 1 / 2 / 64 candidates"""
    groups, wants = [], []
    for ci in by_metric(gold)[metric]:
        g, w = case_group(gold, ci)
        groups.append(g); wants.append(w)
    assert len(groups) > 6
    run(dsp, groups, metric)
    check(groups, wants)


def repeat_case(z, ci, n, **over):
    P, dist, cb, cr, blk, rates, _ = mg.case_of(z, ci)
    idx = (np.arange(n) * 7 + 3) % len(dist)
    P = dict(P, **over)
    return P, dist[idx], None if cb is None else cb[idx], None if cr is None else cr[idx], blk[idx], rates


def test_block_counts_around_a_workgroup(dsp, gold):
    """8x8 with 1, 5 and 67 blocks (a wave per block, four per workgroup: a lone block, a second workgroup of one wave, 17 workgroups with a
    ragged last one), with and without the optional outputs; an empty group between them"""
    ci = mg.CASE_NAMES.index("8x8_sad_nfl12")
    groups, wants = [], []
    for n, gather, allc in ((1, True, True), (5, False, True), (67, True, False), (67, False, False)):
        g, w = pick_group(*repeat_case(gold, ci, n), gather=gather, all_cost=allc, salt=n)
        groups.append(g); wants.append(w)
    empty = dict(groups[0], nblocks=0)
    run(dsp, [groups[0], empty] + groups[1:], SAD)
    check(groups, wants)
    run(dsp, [], SAD)


def test_groups_large_enough_for_several_blocks_per_wave(dsp, gold):
    """the host gives a wave 2, 3 and 4 blocks in turn once a group has more blocks than the device holds waves (32 per CU): the
    fixture's 4x4 blocks repeated to just above 2, 3 and 4 times that many, each with a ragged last wave"""
    slots = torch.cuda.get_device_properties(0).multi_processor_count * 32
    ci = mg.CASE_NAMES.index("4x4_sad_nfl3")
    groups, wants = [], []
    for k in (2, 3, 4):
        g, w = pick_group(*repeat_case(gold, ci, k * slots + 2 * k + 1), salt=k)
        groups.append(g); wants.append(w)
    run(dsp, groups, SAD)
    check(groups, wants)


@pytest.mark.parametrize("metric,name", [(SAD, "8x8_sad_nfl3"), (SSD, "8x8_ssd_nfl12")])
def test_lambdas(dsp, gold, metric, name):
    ci = mg.CASE_NAMES.index(name)
    groups, wants = [], []
    for lam in mg.LAMBDAS:
        g, w = pick_group(*repeat_case(gold, ci, 12, **{"lambda": lam}), salt=lam % 50)
        groups.append(g); wants.append(w)
    assert len({int(w["cost"][0, 0]) for w in wants}) == 3
    run(dsp, groups, metric)
    check(groups, wants)


def test_ties_every_output_equal(dsp, gold):
    """all rate tables zero, distortions from three values: most costs collide, and the order the walk leaves them in is the result"""
    groups, wants = [], []
    for name in ("syn_ties3_nfl3", "syn_ties3_nfl12", "8x8_sad_ties"):
        g, w = case_group(gold, mg.CASE_NAMES.index(name))
        groups.append(g); wants.append(w)
        assert all(len(set(row.tolist())) <= 3 for row in w["all_cost"]) or name == "8x8_sad_ties"
    run(dsp, groups, SAD)
    check(groups, wants)


def test_wrapper_allocates_the_outputs(dsp, gold):
    ci = mg.CASE_NAMES.index("4x16_sad_nfl3")
    g, w = case_group(gold, ci)
    out = dsp.fast_pick(g["dist"], g["blk"], g["rates"], g["tx_size"], g["bsize"], g["bsize_uv"], g["modes"], g["deltas"], g["uv_modes"], g["uv_deltas"],
                        g["nfl"], g["lambda"], SAD, use_angle_delta=g["use_angle_delta"], slice_is_intra=g["slice_is_intra"], intrabc_bits=g["intrabc_bits"],
                        dist_cb=g["dist_cb"], dist_cr=g["dist_cr"], pred=g["pred"], src_xy=g["src_xy"], want_all_cost=True)
    torch.cuda.synchronize()
    check([dict(g, **out)], [w])


def test_out_of_range_context_bytes_are_clamped(dsp, gold):
    """bytes above the tables' ranges in some blocks: their costs are those of the clamped values (what the code's min() gives), every
    other block's results are unchanged"""
    for name, metric in (("8x8_sad_nfl12", SAD), ("8x8_ssd_nfl3", SSD)):
        P, dist, cb, cr, blk, rates = repeat_case(gold, mg.CASE_NAMES.index(name), 12)
        good, w_good = pick_group(P, dist, cb, cr, blk, rates, salt=1)
        wild = blk.copy()
        for b, k in ((2, "top_mode"), (5, "left_mode"), (7, "skip_mode_ctx"), (9, "is_inter_ctx")):
            wild[k][b] = 255
        wild["top_mode"][10], wild["left_mode"][10], wild["skip_mode_ctx"][10], wild["is_inter_ctx"][10] = 13, 200, 3, 4
        bad, w_bad = pick_group(P, dist, cb, cr, wild, rates, salt=1)
        run(dsp, [good, bad], metric)
        check([good, bad], [w_good, w_bad])
        same = [b for b in range(12) if b not in (2, 5, 7, 9, 10)]
        for k in ("cand", "sorted", "cost", "rate", "ref_fast_cost", "all_cost", "pred_out"):
            assert torch.equal(good[k][same], bad[k][same]), k


def untouched(g):
    fill = poison.fill_value(torch.uint8)
    return all(bool((g[k].view(torch.uint8) == fill).all()) for k in OUT_DTYPES if g.get(k) is not None)


def test_invalid_arguments_return_before_any_launch(dsp, gold):
    good, w = case_group(gold, mg.CASE_NAMES.index("8x8_sad_nfl12"))
    other, _ = case_group(gold, mg.CASE_NAMES.index("4x4_sad_nfl3"))
    off = lambda k, nb: good[k].reshape(-1).view(torch.uint8)[nb:]
    C = len(good["modes"])
    sub = lambda k, i, v: dict({k: [v if j == i else x for j, x in enumerate(good[k])]})
    cases = [("ncand 0", dict(ncand=0)), ("ncand 65", dict(ncand=65)), ("nfl 0", dict(nfl=0)), ("nfl 41", dict(nfl=41)),
             ("mode 13", sub("modes", 4, 13)), ("uv mode 14", sub("uv_modes", C - 1, 14)), ("delta 4", sub("deltas", 2, 4)), ("delta -4", sub("deltas", 2, -4)),
             ("uv delta 4", sub("uv_deltas", 0, 4)), ("tx_size 19", dict(tx_size=19)), ("tx_size -1", dict(tx_size=-1)), ("bsize 22", dict(bsize=22)),
             ("bsize_uv -1", dict(bsize_uv=-1)), ("negative dequant", dict(ac_dequant_q3=-8)), ("nblocks * ncand too large", dict(nblocks=0x4000000)),
             ("NULL dist", dict(dist=None)), ("NULL blk", dict(blk=None)), ("NULL rates", dict(rates=None)), ("NULL cand", dict(cand=None)),
             ("NULL sorted", dict(sorted=None)), ("NULL cost", dict(cost=None)), ("NULL rate", dict(rate=None)), ("NULL ref_fast_cost", dict(ref_fast_cost=None)),
             ("pred_out without pred", dict(pred=None)), ("src_xy_out without src_xy", dict(src_xy=None)), ("pred_out is pred", dict(pred_out=good["pred"])),
             ("pred 8-byte aligned", dict(pred=off("pred", 8))), ("pred_out 4-byte aligned", dict(pred_out=off("pred_out", 4))),
             ("dist 4-byte aligned", dict(dist=off("dist", 4))), ("dist_cb 4-byte aligned", dict(dist_cb=off("dist_cb", 4))),
             ("cost 4-byte aligned", dict(cost=off("cost", 4))), ("blk 4-byte aligned", dict(blk=off("blk", 4))), ("all_cost 2-byte aligned", dict(all_cost=off("all_cost", 2))),
             ("ref_fast_cost 4-byte aligned", dict(ref_fast_cost=off("ref_fast_cost", 4))), ("rate 2-byte aligned", dict(rate=off("rate", 2))),
             ("rates 1-byte aligned", dict(rates=off("rates", 1))), ("src_xy_out 2-byte aligned", dict(src_xy_out=off("src_xy_out", 2)))]
    for name, change in cases:
        bad = dict(good, **change)
        for order in ([other, bad], [bad, other]):
            assert dsp.fast_pick_frame(order, SAD) == INVALID, name
            torch.cuda.synchronize()
            assert untouched(good) and untouched(other), name
    assert dsp.fast_pick_frame([good], 2) == INVALID                           # metric
    # an empty group's size and list are validated too
    for change in (dict(tx_size=19), dict(nfl=0), dict(modes=[13] + good["modes"][1:])):
        assert dsp.fast_pick_frame([other, dict(good, nblocks=0, **change)], SAD) == INVALID, change
    assert dsp.lib.svt_hip_fast_pick_frame(None, 1, 0, None) == INVALID and dsp.lib.svt_hip_fast_pick_frame(None, -1, 0, None) == INVALID
    torch.cuda.synchronize()
    assert untouched(good) and untouched(other)
    run(dsp, [good], SAD)
    check([good], [w])


# ---- the whole fast search in one call, and the chain into the transform-type search ---------------------------------------------------
def to_plane(src):
    """dense blocks [n, H, W] -> a plane with the blocks side by side at odd origins, its stride, and xy = x | y << 16"""
    n, h, w = src.shape
    stride = n * (w + 1) + 3
    plane = np.zeros((h + 2, stride), np.uint8)
    xy = np.zeros(n, np.uint32)
    for i in range(n):
        x = 1 + i * (w + 1)
        plane[1:1 + h, x:x + w] = src[i]
        xy[i] = x | 1 << 16
    return plane, stride, xy


def loop_inputs(fl, s, order=None):
    """a fast-loop group dict (no outputs) of the blocks of fast_loop.npz's size s, the source as a plane"""
    idx = np.arange(12) if order is None else np.asarray(order)
    plane, stride, xy = to_plane(fl[f"s{s}_src"][idx])
    return dict(src=dev(plane), src_stride=stride, src_xy=dev(xy), top=dev(fl[f"s{s}_top"][idx][:, 15:15 + PITCH]), left=dev(fl[f"s{s}_left"][idx][:, 15:15 + PITCH]), blocks=dev(fl[f"s{s}_blk"][idx]),
                nblocks=len(idx), tx_size=s, modes=[int(v) for v in fl[f"s{s}_modes"]], deltas=[int(v) for v in fl[f"s{s}_deltas"]])


def pick_params(s, modes, deltas, uv_modes, nfl, metric, rng):
    bsize, bsize_uv = mg.bsizes_of_tx(s)
    P = dict(tx_size=s, bsize=bsize, bsize_uv=bsize_uv, modes=np.array(modes, np.uint8), deltas=np.array(deltas, np.int8), uv_modes=np.array(uv_modes, np.uint8),
             uv_deltas=np.zeros(len(modes), np.int8), use_angle_delta=int(min(TX_W[s], TX_H[s]) >= 8), nfl=nfl, slice_is_intra=1, ac_dequant_q3=156, intrabc_bits=0,
             metric=metric)
    P["lambda"] = 29041
    blk = np.zeros(12, mg.BLK_DTYPE)
    blk["top_mode"], blk["left_mode"], blk["has_chroma"] = rng.integers(0, 13, 12), rng.integers(0, 13, 12), rng.integers(0, 2, 12)
    return P, blk, mg.make_rates("rand", rng)


def pick_dict(P, blk, rates, n, C, with_outputs=True):
    """the pick part of a search group: parameters, contexts and fresh poisoned outputs (the per-candidate arrays come from the fast loop)"""
    N, w, h = min(P["nfl"], C), TX_W[P["tx_size"]], TX_H[P["tx_size"]]
    g = dict(bsize=P["bsize"], bsize_uv=P["bsize_uv"], uv_modes=[int(v) for v in P["uv_modes"]], uv_deltas=[int(v) for v in P["uv_deltas"]], nfl=P["nfl"],
             use_angle_delta=P["use_angle_delta"], slice_is_intra=P["slice_is_intra"], ac_dequant_q3=P["ac_dequant_q3"], intrabc_bits=P["intrabc_bits"],
             blk=dev(blk.view(np.uint8).reshape(-1, 8)), rates=dev(rates))
    g["lambda"] = P["lambda"]
    if with_outputs:
        for k, shp in dict(cand=(n, N), sorted=(n, N), cost=(n, N), rate=(n, N, 2), ref_fast_cost=(n,), all_cost=(n, C), pred_out=(n, N, h, w), src_xy_out=(n, N)).items():
            g[k] = poison.tensor(shp, OUT_DTYPES[k], DEV)
    return g


def search_setup(metric):
    """two search groups' ingredients: 4x4 luma (13 candidates) with 4x8 chroma planes, 8x16 luma (61 candidates) without chroma"""
    fl = np.load(FAST_LOOP)
    rng = np.random.default_rng(77)
    out = []
    for s, chroma, nfl in ((0, 5, 3), (7, None, 12)):
        luma = loop_inputs(fl, s)
        cb = loop_inputs(fl, chroma) if chroma is not None else None
        cr = loop_inputs(fl, chroma, np.arange(12)[::-1]) if chroma is not None else None
        uv = cb["modes"] if cb is not None else [0] * len(luma["modes"])
        P, blk, rates = pick_params(s, luma["modes"], luma["deltas"], uv, nfl, metric, rng)
        out.append((luma, cb, cr, P, blk, rates))
    return fl, out


def by_hand(dsp, setup, metric):
    """the calls enqueued separately, every per-candidate array kept -> list of (luma, cb, cr, pick) dicts"""
    res = []
    for luma, cb, cr, P, blk, rates in setup:
        n, C, s = luma["nblocks"], len(luma["modes"]), luma["tx_size"]
        L = dict(luma, dist=poison.tensor((n, C), torch.int64, DEV), pred=poison.tensor((n, C, TX_H[s], TX_W[s]), torch.uint8, DEV))
        planes = [L]
        CB = CR = None
        if cb is not None:
            CB, CR = dict(cb, dist=poison.tensor((n, C), torch.int64, DEV)), dict(cr, dist=poison.tensor((n, C), torch.int64, DEV))
            planes += [CB, CR]
        assert dsp.intra_fast_loop_frame(planes, metric, 0) == 0, dsp.lib.svt_hip_last_error()
        pk = dict(pick_dict(P, blk, rates, n, C), tx_size=s, nblocks=n, modes=luma["modes"], deltas=luma["deltas"], dist=L["dist"], pred=L["pred"], src_xy=luma["src_xy"],
                  dist_cb=CB["dist"] if CB else None, dist_cr=CR["dist"] if CR else None)
        assert dsp.fast_pick_frame([pk], metric) == 0, dsp.lib.svt_hip_last_error()
        res.append((L, CB, CR, pk))
    torch.cuda.synchronize()
    return res


def search_groups(setup, keep):
    groups = []
    for luma, cb, cr, P, blk, rates in setup:
        n, C, s = luma["nblocks"], len(luma["modes"]), luma["tx_size"]
        L, CB, CR = dict(luma), (dict(cb) if cb else None), (dict(cr) if cr else None)
        if keep:
            L["dist"], L["pred"] = poison.tensor((n, C), torch.int64, DEV), poison.tensor((n, C, TX_H[s], TX_W[s]), torch.uint8, DEV)
            if CB:
                CB["dist"], CR["dist"] = poison.tensor((n, C), torch.int64, DEV), poison.tensor((n, C), torch.int64, DEV)
        groups.append(dict(luma=L, cb=CB, cr=CR, pick=pick_dict(P, blk, rates, n, C)))
    return groups


PICK_OUTS = ("cand", "sorted", "cost", "rate", "ref_fast_cost", "all_cost", "pred_out", "src_xy_out")


@pytest.mark.parametrize("metric", [SAD, SSD])
def test_search_frame_equals_the_calls_by_hand_and_the_restatement(dsp, metric):
    fl, setup = search_setup(metric)
    hand = by_hand(dsp, setup, metric)
    kept, lean = search_groups(setup, True), search_groups(setup, False)
    assert dsp.intra_fast_search_scratch_bytes(kept) == 0
    assert dsp.intra_fast_search_frame(kept, metric, None, 0) == 0, dsp.lib.svt_hip_last_error()
    need = dsp.intra_fast_search_scratch_bytes(lean)
    a16 = lambda v: (v + 15) // 16 * 16
    assert need == sum(a16(g["luma"]["nblocks"] * len(g["luma"]["modes"]) * 8) * (3 if g["cb"] else 1) +
                       g["luma"]["nblocks"] * len(g["luma"]["modes"]) * TX_W[g["luma"]["tx_size"]] * TX_H[g["luma"]["tx_size"]] for g in lean)
    scratch = poison.tensor((need,), torch.uint8, DEV)
    assert dsp.intra_fast_search_frame(lean, metric, scratch, 0) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()
    for (L, CB, CR, pk), gk, gl, (luma, cb, cr, P, blk, rates) in zip(hand, kept, lean, setup):
        s = luma["tx_size"]
        poison.assert_written([pk[k] for k in PICK_OUTS] + [L["dist"], L["pred"]])
        assert torch.equal(L["dist"], gk["luma"]["dist"]) and torch.equal(L["pred"], gk["luma"]["pred"]), s
        for k in PICK_OUTS:
            assert torch.equal(pk[k], gk["pick"][k]) and torch.equal(pk[k], gl["pick"][k]), (s, k)
        # the fast loop's distortions are the reference's (fast_loop.npz), the pick's results the restatement's on them
        dist = L["dist"].cpu().numpy().view(np.uint64)
        assert np.array_equal(dist, fl[f"s{s}_{'ssd_c' if metric == SSD else 'sad'}"]), s
        dcb = CB["dist"].cpu().numpy().view(np.uint64) if CB else None
        dcr = CR["dist"].cpu().numpy().view(np.uint64) if CR else None
        want = mg.np_fast_pick(P, dist, dcb, dcr, blk, rates)
        want["pred_out"] = mg.np_gather(want["cand"], L["pred"].cpu().numpy())
        want["src_xy_out"] = np.repeat(luma["src_xy"].cpu().numpy().view(np.uint32)[:, None], want["cand"].shape[1], axis=1)
        check([dict(pk, tx_size=s)], [want])


def reference_search_groups(z, metric):
    """the cases of fast_search_ref.npz of one metric as search groups (every per-candidate array kept, every output poisoned), and what the
    reference's whole function produced for them"""
    groups, wants = [], []
    for ci in range(ms.NCASES):
        P, blk, rates, extra, want = ms.case_of(z, ci)
        if P["metric"] != metric:
            continue
        n, C, s = len(blk), len(P["modes"]), P["tx_size"]
        xy = (extra["xy"][:, 0].astype(np.uint32) | extra["xy"][:, 1].astype(np.uint32) << 16).astype(np.uint32)
        luma = dict(src=dev(extra["src"]), src_stride=extra["src"].shape[1], src_xy=dev(xy), top=dev(extra["top"]), left=dev(extra["left"]), blocks=dev(extra["iblk"]),
                    nblocks=n, tx_size=s, modes=[int(v) for v in P["modes"]], deltas=[int(v) for v in P["deltas"]],
                    dist=poison.tensor((n, C), torch.int64, DEV), pred=poison.tensor((n, C, TX_H[s], TX_W[s]), torch.uint8, DEV))
        groups.append(dict(luma=luma, cb=None, cr=None, pick=pick_dict(P, blk, rates, n, C)))
        wants.append(dict(want, src_xy_out=np.repeat(xy[:, None], want["cand"].shape[1], axis=1)))
    return groups, wants


def check_against_the_reference(groups, wants):
    for g, w in zip(groups, wants):
        s = g["luma"]["tx_size"]
        poison.assert_written([g["pick"][k] for k in PICK_OUTS] + [g["luma"]["dist"], g["luma"]["pred"]])
        assert np.array_equal(g["luma"]["dist"].cpu().numpy().view(np.uint64), w["dist"]), s          # luma_fast_distortion of every candidate
        check([dict(g["pick"], tx_size=s)], [{k: w[k] for k in PICK_OUTS}])
        # the gathered predictions are the fast loop's own of the surviving candidates
        assert np.array_equal(mg.np_gather(w["cand"], g["luma"]["pred"].cpu().numpy()), w["pred_out"]), s


@pytest.mark.parametrize("metric", [SAD, SSD])
def test_search_frame_equals_the_reference_whole_function(dsp, metric):
    """svt_hip_intra_fast_search_frame on tests/golden/fast_search_ref.npz, every case of the metric as the groups of one call: d_cand,
    d_sorted (as slots), d_cost, d_rate, d_ref_fast_cost, d_all_cost, the luma distortions and the gathered predictions must equal what
    the reference's inject_intra_candidates -> perform_fast_loop (ProductMdFastPuPrediction -> av1_predict_intra_block, the AVX2 table
    entries, av1_intra_fast_cost) -> sort_fast_loop_candidates left in its buffers.  Integers, no tolerance.  Eagerly, then captured into
    a graph and replayed once over re-poisoned outputs."""
    groups, wants = reference_search_groups(np.load(ms.OUT), metric)
    assert len(groups) >= 4
    assert dsp.intra_fast_search_scratch_bytes(groups) == 0
    arr = dsp.make_intra_fast_search_groups(groups)
    assert dsp.intra_fast_search_frame(arr, metric, None, 1) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()
    check_against_the_reference(groups, wants)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert dsp.intra_fast_search_frame(arr, metric, None, 1) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.current_stream().wait_stream(side)
    for g in groups:
        for t in [g["pick"][k] for k in PICK_OUTS] + [g["luma"]["dist"], g["luma"]["pred"]]:
            t.view(torch.uint8).fill_(poison.fill_value(torch.uint8))
    graph.replay()
    torch.cuda.synchronize()
    check_against_the_reference(groups, wants)


def test_search_frame_rejects_a_small_scratch_and_bad_stage_arguments(dsp):
    _, setup = search_setup(SAD)
    lean = search_groups(setup, False)
    need = dsp.intra_fast_search_scratch_bytes(lean)
    scratch = poison.tensor((need,), torch.uint8, DEV)
    fill = poison.fill_value(torch.uint8)
    clean = lambda: bool((scratch == fill).all()) and all(untouched(g["pick"]) for g in lean)
    assert dsp.intra_fast_search_frame(lean, SAD, scratch[:need - 16], 0) == INVALID
    assert dsp.intra_fast_search_frame(lean, SAD, scratch[8:], 0) == INVALID          # not 16-byte aligned (and short)
    assert dsp.intra_fast_search_frame(lean, SAD, None, 0) == INVALID
    last = lean[1]
    for change in (dict(luma=dict(last["luma"], top=None)), dict(luma=dict(last["luma"], modes=[13] + last["luma"]["modes"][1:])),
                   dict(pick=dict(last["pick"], cand=None)), dict(pick=dict(last["pick"], nfl=41)), dict(pick=dict(last["pick"], rates=None))):
        assert dsp.intra_fast_search_frame([lean[0], dict(last, **change)], SAD, scratch, 0) == INVALID, list(change)
    first = lean[0]
    assert dsp.intra_fast_search_frame([dict(first, cb=dict(first["cb"], left=None)), last], SAD, scratch, 0) == INVALID          # a chroma stage argument
    assert dsp.intra_fast_search_frame(lean, 2, scratch, 0) == INVALID              # metric
    assert dsp.intra_fast_search_frame(lean, SAD, scratch, 7) == INVALID            # flavour
    torch.cuda.synchronize()
    assert clean()
    assert dsp.intra_fast_search_frame(lean, SAD, scratch, 0) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()
    assert not clean()


def test_search_frame_graph_capture_and_one_replay(dsp):
    _, setup = search_setup(SAD)
    lean = search_groups(setup, False)
    need = dsp.intra_fast_search_scratch_bytes(lean)
    scratch = poison.tensor((need,), torch.uint8, DEV)
    arr = dsp.make_intra_fast_search_groups(lean)
    assert dsp.intra_fast_search_frame(arr, SAD, scratch, 0) == 0, dsp.lib.svt_hip_last_error()      # eager, and warm: nothing is created inside the capture
    torch.cuda.synchronize()
    eager = [{k: g["pick"][k].clone() for k in PICK_OUTS} for g in lean]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert dsp.intra_fast_search_frame(arr, SAD, scratch, 0) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.current_stream().wait_stream(side)
    for g in lean:
        for k in PICK_OUTS:
            g["pick"][k].view(torch.uint8).fill_(0x5A)
    scratch.fill_(0x5A)
    graph.replay()
    torch.cuda.synchronize()
    for g, e in zip(lean, eager):
        for k in PICK_OUTS:
            assert torch.equal(g["pick"][k], e[k]), (g["luma"]["tx_size"], k)


def test_chain_into_the_transform_type_search(dsp):
    """fast loop -> pick -> svt_hip_tx_search_frame on d_pred_out / d_src_xy_out as they lie (nblocks * n full-loop blocks), against the
    same search on a host-side gather of the downloaded arrays"""
    _, setup = search_setup(SAD)
    hand = by_hand(dsp, setup, SAD)
    qrow = {k: np.ascontiguousarray(v[60]) for k, v in svtlibs.quant_tables(8).items()}
    rng = np.random.default_rng(78)
    for (L, _, _, pk), (luma, _, _, P, _, _) in zip(hand, setup):
        s, n = luma["tx_size"], luma["nblocks"]
        N = pk["cand"].shape[1]
        nb = n * N
        types = [t for t in range(16) if txfm_allowed(s, t)][:4]
        nc = min(TX_W[s], 32) * min(TX_H[s], 32)
        cc, ec = mgc.tables_of(s)
        common = dict(tx_size=s, tx_types=types, nblocks=nb, src=luma["src"], src_stride=luma["src_stride"],
                      iscan=dev(np.stack([svtlibs.scan_tables(s, t)[1] for t in types])), txb_skip_ctx=dev(rng.integers(0, 13, nb).astype(np.uint8)),
                      dc_sign_ctx=dev(rng.integers(0, 3, nb).astype(np.uint8)), type_bits=dev(rng.integers(0, 1 << 12, (nb, len(types))).astype(np.int32)),
                      coeff_cost=dev(cc), eob_cost=dev(ec))
        common["lambda"] = 29041
        outs = lambda: dict(decision=poison.tensor((nb, 40), torch.uint8, DEV), best_qcoeff=poison.tensor((nb, nc), torch.int32, DEV))
        on_dev = dict(common, pred=pk["pred_out"], src_xy=pk["src_xy_out"], **outs())
        cand = pk["cand"].cpu().numpy()
        host_pred = mg.np_gather(cand, L["pred"].cpu().numpy())
        host_xy = np.repeat(luma["src_xy"].cpu().numpy()[:, None], N, axis=1)
        on_host = dict(common, pred=dev(host_pred), src_xy=dev(host_xy), **outs())
        for g in (on_dev, on_host):
            need = dsp.tx_search_scratch_bytes([g])
            g["scratch"] = poison.tensor((need,), torch.uint8, DEV)
            assert dsp.tx_search_frame([g], qrow, g["scratch"], 1) == 0, dsp.lib.svt_hip_last_error()
        torch.cuda.synchronize()
        poison.assert_written([on_dev["decision"], on_dev["best_qcoeff"]])
        assert torch.equal(on_dev["decision"], on_host["decision"]) and torch.equal(on_dev["best_qcoeff"], on_host["best_qcoeff"]), s
        assert bool((on_dev["best_qcoeff"] != 0).any())
