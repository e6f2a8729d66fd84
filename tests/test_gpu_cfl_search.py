"""GPU: the CfL alpha search of mode decision.  svt_hip_cfl_search_frame (the (block, plane, alpha) table) and svt_hip_cfl_decide_frame
(cfl_rd_pick_alpha's walk) against the fixture (tests/golden/cfl_search.npz: every leaf the reference's own function, the walk the
generator's glue, see tests/golden/make_golden_cfl_search.py), and svt_hip_cfl_pick_frame against the two calls enqueued by hand."""
import os
import sys

import numpy as np
import pytest
import torch

import poison
import svtlibs
from poison import poisoned_outputs  # noqa: F401
from svtlibs import TX_H, TX_W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "cfl_search.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_cfl_search as mg  # noqa: E402

INVALID = -2
NSZ = len(mg.SIZES)
TABLES = ("dist", "bits", "eob")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return [mg.size_view(z, si) for si in range(NSZ)]


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint64, np.uint16, np.uint32):                          # torch has the signed types
        a = a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}[a.dtype])
    return torch.from_numpy(a).to(DEV)


def search_group(v, blocks=None, x0=0, extra=0, tables=True):
    """(group dict, expected dict) of one fixture size.  blocks: indices into the size's 24 (default all), laid out on planes in rows of
    up to 7 blocks: chroma origin x = x0 + column * pitch (pitch = the width, or 16 when x0 is set: every origin then is x0 mod 16), rows
    of the planes `extra` samples longer than the picture, the last block row touching each plane's last row"""
    s = int(v["size"])
    w, h = TX_W[s], TX_H[s]
    blocks = np.arange(mg.NBLOCKS) if blocks is None else np.asarray(blocks)
    n = len(blocks)
    cols = min(n, 7)
    rows = (n + cols - 1) // cols
    pitch = max(w, 16) if x0 else w
    cw = x0 + cols * pitch
    cstride, lstride = cw + extra, 2 * cw + 2 * extra + (1 if extra else 0)
    rng = np.random.default_rng(n * 31 + s)
    luma = rng.integers(0, 256, (rows * 2 * h, lstride)).astype(np.uint8)     # what lies between the blocks must not matter
    planes = [[rng.integers(0, 256, (rows * h, cstride)).astype(np.uint8) for _ in range(2)] for _ in range(2)]
    xy = np.zeros(n, np.int32)
    for i, b in enumerate(blocks):
        x, y = x0 + (i % cols) * pitch, (i // cols) * h
        xy[i] = x | (y << 16)
        luma[2 * y:2 * y + 2 * h, 2 * x:2 * x + 2 * w] = v["luma"][b]
        for p in range(2):
            planes[0][p][y:y + h, x:x + w] = v["src"][b, p]
            planes[1][p][y:y + h, x:x + w] = v["pred"][b, p]
    g = dict(tx_size=s, tx_type=mg.DCT_DCT, nblocks=n, luma=dev(luma), luma_stride=lstride, src=tuple(dev(a) for a in planes[0]),
             src_stride=(cstride, cstride), pred=tuple(dev(a) for a in planes[1]), pred_stride=(cstride, cstride), xy=dev(xy),
             iscan=dev(svtlibs.scan_tables(s, mg.DCT_DCT)[1].astype(np.int16)),
             txb_skip_ctx=tuple(dev(v["skip_ctx"][p][blocks]) for p in range(2)), dc_sign_ctx=tuple(dev(v["dc_ctx"][p][blocks]) for p in range(2)),
             coeff_cost=dev(v["coeff_cost"]), eob_cost=dev(v["eob_cost"]))
    if tables:
        g.update(dist=poison.tensor((n, 2, mg.NALPHA, 2), torch.int64, DEV), bits=poison.tensor((n, 2, mg.NALPHA), torch.int64, DEV),
                 eob=poison.tensor((n, 2, mg.NALPHA), torch.int16, DEV))
    want = {fl: dict(dist=v["dist_" + ("avx2" if fl else "c")][blocks], bits=v["bits"][blocks], eob=v["eob"][blocks]) for fl in (0, 1)}
    return g, want


def rows_of(v):
    return mg.qrows_of(v["qrows"], 0), mg.qrows_of(v["qrows"], 1)


def scratch_for(dsp, groups, pick=False):
    nbytes = (dsp.cfl_pick_scratch_bytes if pick else dsp.cfl_search_scratch_bytes)(groups)
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV) if nbytes else None


def run_search(dsp, groups, qrows, flavour):
    rc = dsp.cfl_search_frame(groups, qrows[0], qrows[1], scratch_for(dsp, groups), flavour)
    torch.cuda.synchronize()
    assert rc == 0, dsp.lib.svt_hip_last_error()


def fresh_tables(groups):
    for g in groups:
        if g["nblocks"]:
            n = g["nblocks"]
            g.update(dist=poison.tensor((n, 2, mg.NALPHA, 2), torch.int64, DEV), bits=poison.tensor((n, 2, mg.NALPHA), torch.int64, DEV),
                     eob=poison.tensor((n, 2, mg.NALPHA), torch.int16, DEV))


def check_tables(groups, wants, flavour):
    for g, w in zip(groups, wants):
        for key in TABLES:
            got = g[key].cpu().numpy().view(w[flavour][key].dtype)
            bad = np.argwhere(got != w[flavour][key])
            assert bad.size == 0, (g["tx_size"], key, flavour, len(bad), bad[:6].tolist(), got[tuple(bad[0])], w[flavour][key][tuple(bad[0])])


def test_table_bit_for_bit_nine_sizes_both_flavours(dsp, gold):
    """d_dist, d_bits and d_eob of every fixture block, all nine sizes as nine groups of one call, once per flavour"""
    pairs = [search_group(v) for v in gold]
    groups, wants = [g for g, _ in pairs], [w for _, w in pairs]
    for flavour in (1, 0):
        fresh_tables(groups)
        run_search(dsp, groups, rows_of(gold[0]), flavour)
        check_tables(groups, wants, flavour)


@pytest.mark.parametrize("si", range(NSZ))
def test_block_counts(dsp, gold, si):
    """per size: 1 block; one more than a wave holds; a count that leaves the last workgroup with idle waves (a workgroup's four waves take
    two wave-loads of blocks for both planes: five wave-loads and one block need three workgroups, the last with two idle waves)"""
    v = gold[si]
    bpw = 64 // max(TX_W[int(v["size"])], TX_H[int(v["size"])])
    pairs = [search_group(v, (np.arange(n) * 5 + k) % mg.NBLOCKS) for k, n in enumerate((1, bpw + 1, 4 * bpw + 1))]
    groups, wants = [g for g, _ in pairs], [w for _, w in pairs]
    run_search(dsp, groups, rows_of(v), 1)
    check_tables(groups, wants, 1)


def test_plane_addressing(dsp, gold):
    """strides larger than the width (an odd luma stride among them), origins at x = 4 mod 16, the last block row on the planes' last
    row: every size, 10 blocks each (two block rows, the second one short)"""
    pairs = [search_group(v, (np.arange(10) * 3 + 1) % mg.NBLOCKS, x0=4, extra=9) for v in gold]
    groups, wants = [g for g, _ in pairs], [w for _, w in pairs]
    run_search(dsp, groups, rows_of(gold[0]), 1)
    check_tables(groups, wants, 1)


def test_eighteen_groups_and_an_empty_one(dsp, gold):
    """18 groups cross the per-launch group limit of the search kernel (16); an empty group sits in the middle"""
    pairs = [search_group(gold[k % NSZ], (np.arange(5 + k) * 7 + k) % mg.NBLOCKS) for k in range(18)]
    groups, wants = [g for g, _ in pairs], [w for _, w in pairs]
    empty = dict(tx_size=2, tx_type=0, nblocks=0)
    run_search(dsp, groups[:9] + [empty] + groups[9:], rows_of(gold[0]), 1)
    check_tables(groups, wants, 1)


def test_cb_and_cr_rows_differ(dsp, gold):
    """the fixture's Cb and Cr rows differ (checked here), and the table is right only with each plane's own; then rows whose AC entries
    differ as well, against the restatement: a kernel that reuses one plane's rows fails one of the two"""
    v = gold[1]
    assert not np.array_equal(v["qrows"][0], v["qrows"][1])
    g, w = search_group(v)
    run_search(dsp, [g], rows_of(v), 1)
    check_tables([g], [w], 1)
    fresh_tables([g])
    run_search(dsp, [g], (rows_of(v)[0], rows_of(v)[0]), 1)                  # Cr with Cb's rows: Cb right, Cr wrong somewhere
    got = g["eob"].cpu().numpy().view(np.uint16), g["dist"].cpu().numpy().view(np.uint64)
    assert np.array_equal(got[0][:, 0], w[1]["eob"][:, 0]) and np.array_equal(got[1][:, 0], w[1]["dist"][:, 0])
    assert (got[1][:, 1] != w[1]["dist"][:, 1]).any()
    sub = mg.ac_rows_case(v)                                                 # (pinned to the reference in tests/test_cfl_search_cpu.py)
    t = mg.np_table(sub)
    g, _ = search_group(v, np.arange(sub["luma"].shape[0]))
    run_search(dsp, [g], (mg.qrows_of(sub["qrows"], 0), mg.qrows_of(sub["qrows"], 1)), 1)
    check_tables([g], [{1: dict(dist=t["dist_avx2"], bits=t["bits"], eob=t["eob"])}], 1)


def decide_group(v, flavour="avx2", blocks=None, alphas=True):
    blocks = np.arange(mg.NBLOCKS) if blocks is None else np.asarray(blocks)
    n = len(blocks)
    g = dict(nblocks=n, dist=dev(v["dist_" + flavour][blocks]), bits=dev(v["bits"][blocks]), alpha_rate=dev(v["alpha_rate"]),
             cfl_mode_bits=dev(v["cfl_mode_bits"][blocks]), dc_mode_bits=dev(v["dc_mode_bits"][blocks]),
             decision=poison.tensor((n, 32), torch.uint8, DEV))
    g["lambda"] = int(v["lam"])
    if alphas:
        g.update(alpha_q3_cb=poison.tensor((n,), torch.int32, DEV), alpha_q3_cr=poison.tensor((n,), torch.int32, DEV))
    return g, v["decision_" + flavour].view(mg.DEC_DTYPE).reshape(-1)[blocks]


def check_decisions(groups, wants):
    for g, w in zip(groups, wants):
        got = g["decision"].cpu().numpy().view(mg.DEC_DTYPE).reshape(-1)
        bad = np.flatnonzero(got != w)
        assert bad.size == 0, (bad[:8].tolist(), got[bad[0]], w[bad[0]])
        if g.get("alpha_q3_cb") is not None:
            assert np.array_equal(g["alpha_q3_cb"].cpu().numpy(), w["alpha_q3"][:, 0]) and np.array_equal(g["alpha_q3_cr"].cpu().numpy(), w["alpha_q3"][:, 1])


def test_decide_every_record_and_both_alpha_arrays(dsp, gold):
    """all nine sizes x both flavours' tables in one call (18 groups), the tie block (flat luma, block 0) among them; then 300 blocks (two
    workgroups, the second ragged) and a group whose d_alpha_q3_* are NULL, an empty group between them"""
    pairs = [decide_group(v, fl) for v in gold for fl in ("avx2", "c")]
    groups, wants = [g for g, _ in pairs], [w for _, w in pairs]
    rc = dsp.cfl_decide_frame(groups)
    torch.cuda.synchronize()
    assert rc == 0, dsp.lib.svt_hip_last_error()
    check_decisions(groups, wants)
    assert all(w["uv_mode"][mg.FLAT] == mg.UV_DC_PRED for w in wants)           # all alphas tie: nothing beats DC's cheaper mode
    pairs = [decide_group(gold[2], blocks=(np.arange(300) * 7) % mg.NBLOCKS), decide_group(gold[5], alphas=False)]
    groups, wants = [g for g, _ in pairs], [w for _, w in pairs]
    rc = dsp.cfl_decide_frame([groups[0], dict(nblocks=0), groups[1]])
    torch.cuda.synchronize()
    assert rc == 0, dsp.lib.svt_hip_last_error()
    check_decisions(groups, wants)


def test_pick_equals_search_then_decide(dsp, gold):
    """svt_hip_cfl_pick_frame with every table in the scratch, and with the caller's dist, against the two calls enqueued by hand"""
    sizes = (0, 2, 7)
    hand_s = [search_group(gold[si])[0] for si in sizes]
    run_search(dsp, hand_s, rows_of(gold[0]), 1)
    hand_d = []
    for si, s in zip(sizes, hand_s):
        d, _ = decide_group(gold[si])
        d.update(dist=s["dist"], bits=s["bits"])
        hand_d.append(d)
    assert dsp.cfl_decide_frame(hand_d) == 0
    picks = []
    for k, si in enumerate(sizes):
        g, _ = search_group(gold[si], tables=False)
        d, want = decide_group(gold[si])
        g.update({key: d[key] for key in ("alpha_rate", "cfl_mode_bits", "dc_mode_bits", "decision", "alpha_q3_cb", "alpha_q3_cr", "lambda")})
        if k == 1:
            g["dist"] = poison.tensor((g["nblocks"], 2, mg.NALPHA, 2), torch.int64, DEV)
        picks.append(g)
    q = rows_of(gold[0])
    rc = dsp.cfl_pick_frame(picks, q[0], q[1], scratch_for(dsp, picks, pick=True), 1)
    torch.cuda.synchronize()
    assert rc == 0, dsp.lib.svt_hip_last_error()
    for h, p, si in zip(hand_d, picks, sizes):
        for key in ("decision", "alpha_q3_cb", "alpha_q3_cr"):
            assert torch.equal(h[key], p[key]), (si, key)
        poison.assert_written(h["alpha_q3_cb"], h["alpha_q3_cr"], p["alpha_q3_cb"], p["alpha_q3_cr"], h["decision"].view(torch.int64), p["decision"].view(torch.int64))
    assert torch.equal(picks[1]["dist"], hand_s[1]["dist"])
    poison.assert_written(picks[1]["dist"], hand_s[1]["dist"])
    want = gold[sizes[0]]["decision_avx2"].view(mg.DEC_DTYPE).reshape(-1)
    assert np.array_equal(picks[0]["decision"].cpu().numpy().view(mg.DEC_DTYPE).reshape(-1), want)


def test_invalid_arguments_leave_the_outputs_untouched(dsp, gold):
    v = gold[1]
    q = rows_of(v)

    def refused(change, scratch="ok", qrows=q):
        g, _ = search_group(v, np.arange(3))
        change(g)
        full = scratch_for(dsp, [search_group(v, np.arange(3))[0]])
        sc = {"ok": full, "none": None, "small": full[:full.numel() - 16], "odd": full[8:]}[scratch]
        rc = dsp.cfl_search_frame([g], qrows[0], qrows[1], sc, 1)
        torch.cuda.synchronize()
        assert rc == INVALID, rc
        for key in TABLES:
            assert bool((g[key] == poison.fill_value(g[key].dtype)).all()), key

    refused(lambda g: g.update(tx_size=3))                                    # 32x32
    refused(lambda g: g.update(tx_size=15))                                   # 8x32
    refused(lambda g: g.update(tx_size=17))                                   # a 64-sample side
    refused(lambda g: g.update(tx_size=19))
    refused(lambda g: g.update(tx_type=16))                                   # a type not defined for the size
    refused(lambda g: g.update(luma=None))                                    # a NULL plane
    refused(lambda g: g.update(src=(g["src"][0], None)))
    refused(lambda g: g.update(dist=g["dist"].view(-1)[1:]))                  # a misaligned d_dist (8 bytes off)
    refused(lambda g: g.update(src_stride=(7, 8)))
    refused(lambda g: None, scratch="small")
    refused(lambda g: None, scratch="none")
    refused(lambda g: None, scratch="odd")
    bad_q = dict(q[1]); bad_q["quant_shift"] = np.array([3] * 8, np.int16)
    refused(lambda g: None, qrows=(q[0], bad_q))
    def untouched(g, keys):
        torch.cuda.synchronize()
        for key in keys:
            assert bool((g[key] == poison.fill_value(g[key].dtype)).all()), key

    # an empty group's size is checked too; the decide and the pick refuse the same way
    g, _ = search_group(v, np.arange(3))
    assert dsp.cfl_search_frame([g, dict(tx_size=4, tx_type=0, nblocks=0)], q[0], q[1], scratch_for(dsp, [g]), 1) == INVALID
    untouched(g, TABLES)
    dec_out = ("decision", "alpha_q3_cb", "alpha_q3_cr")
    for change in (lambda d: d.update(bits=None), lambda d: d.update(dist=d["dist"].view(-1)[1:]), lambda d: d.update(alpha_rate=None),
                   lambda d: d.update(cfl_mode_bits=d["cfl_mode_bits"].view(torch.int16)[1:]), lambda d: d.update(nblocks=0x2000000)):
        d, _ = decide_group(v)
        keep = {k: d[k] for k in dec_out}
        change(d)
        assert dsp.cfl_decide_frame([d]) == INVALID
        untouched(keep, dec_out)
    # the pick: no scratch, a scratch that is too small, a bad member of either stage; a good group beside the bad one is not run either
    def pick_groups():
        out = []
        for _ in range(2):
            p, _ = search_group(v, np.arange(3), tables=False)
            d, _ = decide_group(v, blocks=np.arange(3))
            p.update({k: d[k] for k in ("alpha_rate", "cfl_mode_bits", "dc_mode_bits", "lambda") + dec_out})
            out.append(p)
        return out

    full = scratch_for(dsp, pick_groups(), pick=True)
    for change, sc in ((lambda p: None, None), (lambda p: None, full[:full.numel() - 16]), (lambda p: p.update(luma=None), full),
                       (lambda p: p.update(alpha_rate=None), full), (lambda p: p.update(tx_size=3), full)):
        ps = pick_groups()
        change(ps[1])
        assert dsp.cfl_pick_frame(ps, q[0], q[1], sc, 1) == INVALID
        for p in ps:
            untouched(p, dec_out)
