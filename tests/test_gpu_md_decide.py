"""GPU: svt_hip_md_decide_frame (full cost, early exit, best candidate and the winner's arrays per block) against the fixture
(tests/golden/md_decide.npz: the reference's cost functions and product_full_mode_decision, the generator's escape walk) and its numpy
restatement, and svt_hip_md_search_frame (luma transform-type search -> chroma full loop and rate -> decide in one call) against the
stages enqueued by hand."""
import os
import sys

import numpy as np
import pytest
import torch

import poison
import svtlibs
from poison import poisoned_outputs  # noqa: F401
from svtlibs import txfm_allowed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "md_decide.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_coeff_rate as mgc  # noqa: E402
import make_golden_md_decide as mg  # noqa: E402

INVALID = -2
GATHERS = ("best_pred", "best_qcoeff", "best_dqcoeff")
SALT = {"pred": 3, "qcoeff": 7, "dqcoeff": 900001, "inter_blk": 11}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def dev(a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}.get(a.dtype)      # torch has the signed types
    return torch.from_numpy(a.view(view) if view else a).to(DEV)


def plane_sizes(bsize):
    """per plane (w, h, NC)"""
    out = []
    for p in range(3):
        w, h = (mg.BSIZE_W[bsize], mg.BSIZE_H[bsize]) if p == 0 else (max(mg.BSIZE_W[bsize] // 2, 4), max(mg.BSIZE_H[bsize] // 2, 4))
        out.append((w, h, min(w, 32) * min(h, 32)))
    return out


def index_tensor(nb, n, m, salt, dtype):
    """[nb, n, m] on the device, every entry a function of its indices; bytes never hold the poison pattern at every position"""
    i = lambda k, shape: torch.arange(k, dtype=torch.int64, device=DEV).view(shape)
    v = i(nb, (nb, 1, 1)) * 4099 + i(n, (1, n, 1)) * 1031 + i(m, (1, 1, m)) + salt
    return (v % 251 if dtype == torch.uint8 else v + 1).to(dtype).contiguous()


def index_expected(dec, m, salt, dtype, plane=None):
    """the winner's row of index_tensor; with plane (coefficients) zeros where the winner's eob of that plane is 0"""
    nb = len(dec)
    v = np.arange(nb, dtype=np.int64)[:, None] * 4099 + dec["slot"].astype(np.int64)[:, None] * 1031 + np.arange(m, dtype=np.int64)[None, :] + salt
    out = (v % 251).astype(np.uint8) if dtype == torch.uint8 else (v + 1).astype(np.int32)
    if plane is not None:
        out[dec["eob"][:, plane] == 0] = 0
    return out


def case_group(z, k, blocks=None, gathers=("pred", "qcoeff", "dqcoeff", "inter_blk"), outputs=None, full_cost=True):
    """(group dict, expected dict) of fixture case k: blocks (indices into the case's, default all; a block's record depends on the
    block alone, so any selection and repetition keeps the fixture's records)"""
    blocks = np.arange(mg.NBLOCKS) if blocks is None else np.asarray(blocks)
    outputs = gathers if outputs is None else outputs
    nb, n, bsize = len(blocks), int(z[f"c{k}_n"]), int(z[f"c{k}_bsize"])
    dec = mg.decisions(z, k)[blocks]
    g = dict(bsize=bsize, nblocks=nb, n=n, ninter=int(z[f"c{k}_ninter"]), nintra=int(z[f"c{k}_nintra"]), modes=z[f"c{k}_modes"],
             slice_is_intra=int(z[f"c{k}_slice_is_intra"]), full_loop_escape=int(z[f"c{k}_escape"]),
             luma=dev(z[f"c{k}_luma"][blocks]), rate=dev(z[f"c{k}_rate"][blocks]), cand=dev(z[f"c{k}_cand"][blocks]),
             cand_out=dev(z[f"c{k}_cand_out"][blocks]), blk=dev(z[f"c{k}_blk"][blocks]), rates=dev(z["rates"]),
             decision=poison.tensor((nb, 72), torch.uint8, DEV))
    g["lambda"] = int(z[f"c{k}_lam"])
    if int(z[f"c{k}_has_chroma"]):
        for p, c in enumerate(("cb", "cr")):
            g["dist_" + c], g["bits_" + c], g["eob_" + c] = dev(z[f"c{k}_cdist"][p][blocks]), dev(z[f"c{k}_cbits"][p][blocks]), dev(z[f"c{k}_ceob"][p][blocks])
    if int(z[f"c{k}_has_cfl"]):
        g["cfl"] = dev(z[f"c{k}_cfl"][blocks])
    want = dict(decision=dec)
    if full_cost:
        g["full_cost"] = poison.tensor((nb, n), torch.int64, DEV)
        want["full_cost"] = z[f"c{k}_cost"][blocks]
    sizes = plane_sizes(bsize)
    for key in ("pred", "qcoeff", "dqcoeff"):
        if key in gathers:
            dt = torch.uint8 if key == "pred" else torch.int32
            ms = [w * h if key == "pred" else nc for w, h, nc in sizes]
            g[key] = [index_tensor(nb, n, m, SALT[key] + p, dt) for p, m in enumerate(ms)]
            if key in outputs:
                g["best_" + key] = [poison.tensor((nb, m), dt, DEV) for m in ms]
                want["best_" + key] = [index_expected(dec, m, SALT[key] + p, dt, None if key == "pred" else p) for p, m in enumerate(ms)]
    if "inter_blk" in gathers:
        g["inter_blk"] = index_tensor(nb, n, 16, SALT["inter_blk"], torch.uint8)
        if "inter_blk" in outputs:
            g["best_inter_blk"] = poison.tensor((nb, 16), torch.uint8, DEV)
            want["best_inter_blk"] = index_expected(dec, 16, SALT["inter_blk"], torch.uint8)
    return g, want


def run(dsp, groups):
    rc = dsp.md_decide_frame(groups)
    torch.cuda.synchronize()
    assert rc == 0, dsp.lib.svt_hip_last_error()


def check(groups, wants):
    for gi, (g, w) in enumerate(zip(groups, wants)):
        got = g["decision"].cpu().numpy().view(mg.DEC_DTYPE).reshape(-1)
        bad = np.flatnonzero(got != w["decision"])
        assert bad.size == 0, (gi, g["bsize"], g["n"], bad[:8].tolist(), got[bad[0]], w["decision"][bad[0]])
        if "full_cost" in w:
            assert np.array_equal(g["full_cost"].cpu().numpy().view(np.uint64), w["full_cost"]), (gi, "full_cost")
        for key in GATHERS:
            for p, exp in enumerate(w.get(key, ())):
                out = g[key][p].cpu().numpy()
                bad = np.argwhere(out != exp)
                assert bad.size == 0, (gi, g["bsize"], key, p, bad[:8].tolist(), out[tuple(bad[0])], exp[tuple(bad[0])])
        if "best_inter_blk" in w:
            assert np.array_equal(g["best_inter_blk"].cpu().numpy(), w["best_inter_blk"]), (gi, "best_inter_blk")


def test_golden_fixture_all_cases_in_one_call(dsp, gold):
    """every fixture case record for record with every gather on, then each again with its blocks repeated in another order (131 or 37
    blocks: a last wave-unit that is not full; 14 groups: two launches)"""
    groups, wants = [], []
    for k in range(mg.NCASES):
        g, w = case_group(gold, k)
        groups.append(g); wants.append(w)
    for k in range(mg.NCASES):
        g, w = case_group(gold, k, (np.arange(37 if k == 4 else 131) * 7) % mg.NBLOCKS)     # (64x64 with 40 slots: fewer blocks, the arrays are large)
        groups.append(g); wants.append(w)
    run(dsp, groups)
    check(groups, wants)
    zero = [sum(int((w["decision"]["eob"][:, p] == 0).sum()) for w in wants) for p in range(3)]
    cut = sum(int((w["decision"]["count"] < g["n"]).sum()) for g, w in zip(groups, wants))
    assert all(zero) and cut > 0                                             # the zero-fill path of every plane's gather ran; escapes fired


@pytest.mark.parametrize("k,unit", [(3, 64), (4, 2)], ids=["4x4_unit64", "64x64_unit2"])
def test_one_below_at_and_above_a_wave_unit_and_a_workgroup(dsp, gold, k, unit):
    """the largest wave-unit (64 blocks of 4x4 with n = 3) and the smallest (2 blocks of 64x64): nblocks 1, unit - 1, unit, unit + 1, and
    one more than the four units of a workgroup"""
    groups, wants = [], []
    for nb in sorted({1, unit - 1, unit, unit + 1, 4 * unit + 1}):
        g, w = case_group(gold, k, (np.arange(nb) * 5 + 1) % mg.NBLOCKS)
        groups.append(g); wants.append(w)
    run(dsp, groups)
    check(groups, wants)


def test_two_block_sizes_with_an_empty_group_between(dsp, gold):
    """4x4 (every NC 16) and 32x32 (luma NC 1024, chroma NC 256): the three planes' gathers run with different log2 sizes in one launch"""
    a, wa = case_group(gold, 3, np.arange(70) % mg.NBLOCKS)
    b, wb = case_group(gold, 2, np.arange(9))
    empty = dict(bsize=6, nblocks=0, n=3, ninter=1, nintra=0)
    run(dsp, [a, empty, b])
    check([a, b], [wa, wb])
    run(dsp, [])


def test_gathers_are_independent(dsp, gold):
    """any subset of the gathers; an input without its output is read by nobody; no gather at all; no d_full_cost"""
    groups, wants = [], []
    for k, gathers, outputs, fc in ((0, ("pred",), None, True), (1, ("qcoeff", "inter_blk"), None, False), (0, ("pred", "qcoeff", "dqcoeff"), ("dqcoeff",), True),
                                    (2, (), None, False), (6, ("inter_blk", "dqcoeff"), ("inter_blk",), True)):
        g, w = case_group(gold, k, np.arange(19), gathers=gathers, outputs=outputs, full_cost=fc)
        groups.append(g); wants.append(w)
    # one plane only: Cb's coefficients without luma's and Cr's
    g, w = case_group(gold, 1, np.arange(11), gathers=("qcoeff",))
    for key in ("qcoeff", "best_qcoeff"):
        g[key] = [None, g[key][1], None]
    w["best_qcoeff"] = [None, w["best_qcoeff"][1], None]
    groups.append(g); wants.append(w)
    run(dsp, groups)
    for g, w in zip(groups, wants):
        for key in GATHERS:
            if key in w:
                keep = [p for p, e in enumerate(w[key]) if e is not None]
                w[key] = [w[key][p] for p in keep]; g[key] = [g[key][p] for p in keep]
    check(groups, wants)


def test_graph_capture_and_two_replays(dsp, gold):
    groups, wants = [], []
    for k in (0, 3, 2):
        g, w = case_group(gold, k)
        groups.append(g); wants.append(w)
    arr = dsp.make_md_decide_groups(groups)
    run(dsp, arr)                                                         # warm: nothing is created inside the capture
    check(groups, wants)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert dsp.md_decide_frame(arr) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for g in groups:
            for t in outputs_of(g):
                t.view(torch.uint8).fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        check(groups, wants)


def outputs_of(g):
    out = [g[k] for k in ("decision", "full_cost", "best_inter_blk") if g.get(k) is not None]
    for key in GATHERS:
        out += [t for t in g.get(key) or () if t is not None]
    return out


def untouched(g):
    fill = poison.fill_value(torch.uint8)
    return all(bool((t.view(torch.uint8) == fill).all()) for t in outputs_of(g))


def invalid_cases(g):
    """(name, changes to a valid group) that svt_hip_md_decide_frame must reject"""
    off = lambda t, n: t.reshape(-1).view(torch.uint8)[n:]                 # the same buffer, n bytes in
    plane = lambda key, p, t: [t if q == p else x for q, x in enumerate(g[key])]
    cases = [("bsize 13", dict(bsize=13)), ("bsize 14", dict(bsize=14)), ("bsize 15", dict(bsize=15)), ("bsize 22", dict(bsize=22)), ("bsize -1", dict(bsize=-1)),
             ("n 0", dict(n=0)), ("n 41", dict(n=41)), ("no candidates", dict(ninter=0, nintra=0)), ("65 candidates", dict(ninter=60, nintra=5)),
             ("ninter -1", dict(ninter=-1)), ("escape 3", dict(full_loop_escape=3)), ("mode 13", dict(modes=[13] * g["nintra"])),
             ("nblocks * n too large", dict(nblocks=0x7fffffff // g["n"] + 1)),
             ("NULL luma", dict(luma=None)), ("NULL rate", dict(rate=None)), ("NULL cand", dict(cand=None)), ("NULL blk", dict(blk=None)),
             ("NULL rates", dict(rates=None)), ("NULL decision", dict(decision=None)), ("NULL cand_out", dict(cand_out=None)),
             ("Cb without Cr", dict(dist_cr=None, bits_cr=None, eob_cr=None)), ("no Cb eob", dict(eob_cb=None)),
             ("best_inter_blk without inter_blk", dict(inter_blk=None)), ("best_inter_blk is inter_blk", dict(best_inter_blk=g["inter_blk"])),
             ("luma 4-byte aligned", dict(luma=off(g["luma"], 4))), ("dist_cb 4-byte aligned", dict(dist_cb=off(g["dist_cb"], 4))),
             ("bits_cr 4-byte aligned", dict(bits_cr=off(g["bits_cr"], 4))), ("eob_cr 1-byte aligned", dict(eob_cr=off(g["eob_cr"], 1))),
             ("cfl 4-byte aligned", dict(cfl=off(g["cfl"], 4))), ("decision 4-byte aligned", dict(decision=off(g["decision"], 4))),
             ("full_cost 4-byte aligned", dict(full_cost=off(g["full_cost"], 4))), ("rate 2-byte aligned", dict(rate=off(g["rate"], 2))),
             ("rates 2-byte aligned", dict(rates=off(g["rates"], 2))), ("blk 2-byte aligned", dict(blk=off(g["blk"], 2))),
             ("inter_blk 8-byte aligned", dict(inter_blk=off(g["inter_blk"], 8))), ("best_inter_blk 8-byte aligned", dict(best_inter_blk=off(g["best_inter_blk"], 8)))]
    for p in range(3):
        for key in ("pred", "qcoeff", "dqcoeff"):
            cases += [(f"best_{key}[{p}] without its input", {key: plane(key, p, None)}),
                      (f"best_{key}[{p}] is its input", {"best_" + key: plane("best_" + key, p, g[key][p])}),
                      (f"{key}[{p}] 8-byte aligned", {key: plane(key, p, off(g[key][p], 8))}),
                      (f"best_{key}[{p}] 8-byte aligned", {"best_" + key: plane("best_" + key, p, off(g["best_" + key][p], 8))})]
    return cases


def test_invalid_arguments_return_before_any_launch(dsp, gold):
    good, w = case_group(gold, 0, np.arange(9))
    other, _ = case_group(gold, 2, np.arange(5))
    for name, change in invalid_cases(good):
        bad = dict(good, **change)
        for order in ([other, bad], [bad, other]):                       # the bad group last: nothing before it may have run
            assert dsp.md_decide_frame(dsp.make_md_decide_groups(order)) == INVALID, name
            torch.cuda.synchronize()
            assert untouched(good) and untouched(other), name
    # an empty group's scalars are validated too
    for change in (dict(bsize=13), dict(n=41), dict(full_loop_escape=3), dict(ninter=0)):
        empty = dict(dict(bsize=3, nblocks=0, n=3, ninter=1, nintra=0), **change)
        assert dsp.md_decide_frame(dsp.make_md_decide_groups([other, empty])) == INVALID, change
    assert dsp.lib.svt_hip_md_decide_frame(None, 1, None) == INVALID and dsp.lib.svt_hip_md_decide_frame(None, -1, None) == INVALID
    torch.cuda.synchronize()
    assert untouched(other) and untouched(good)
    run(dsp, [good])
    check([good], [w])


# ---- the whole decision in one call ---------------------------------------------------------------------------------------------
TX_OF = {(4, 4): 0, (8, 8): 1, (16, 16): 2, (32, 32): 3, (64, 64): 4}
SEARCH = ((0, 12, 5), (9, 3, 3), (12, 2, 2))                               # (bsize, n, nblocks): 4x4, 32x32 (chroma 16x16), 64x64 (chroma 32x32)
LAMBDA = 29041
MD_OUT = ("decision", "full_cost", "best_inter_blk")


def search_inputs(gold):
    """per block size: the survivors' sources and predictions of the three planes, the contexts and cost tables of the stages, and the
    decide's own inputs"""
    rng = np.random.default_rng(4127)
    out = []
    for bsize, n, nb in SEARCH:
        sizes, pairs = plane_sizes(bsize), nb * n
        tx = [TX_OF[(w, h)] for w, h, _ in sizes]
        planes = []
        for p, (w, h, nc) in enumerate(sizes):
            src = np.repeat(rng.integers(0, 256, (nb, 1, h, w)), n, axis=1).reshape(pairs, h, w).astype(np.uint8)      # one source per block
            noise = rng.integers(-12, 13, (pairs, h, w)) * (rng.random((pairs, 1, 1)) < 0.75)                          # some survivors predict exactly
            pred = np.clip(src.astype(np.int32) + noise, 0, 255).astype(np.uint8)
            types = [t for t in range(16) if txfm_allowed(tx[p], t)][:4] if p == 0 else [0]
            cc, ec = mgc.tables_of(tx[p])
            planes.append(dict(tx_size=tx[p], tx_types=types, nblocks=pairs, src=dev(src), pred=dev(pred),
                               iscan=dev(np.stack([svtlibs.scan_tables(tx[p], t)[1] for t in types])),
                               txb_skip_ctx=dev(rng.integers(0, 13, pairs).astype(np.uint8)), dc_sign_ctx=dev(rng.integers(0, 3, pairs).astype(np.uint8)),
                               coeff_cost=dev(cc), eob_cost=dev(ec)))
        planes[0]["type_bits"] = dev(rng.integers(0, 1 << 12, (pairs, len(planes[0]["tx_types"]))).astype(np.int32))
        planes[0]["lambda"] = LAMBDA
        ninter, nintra = 6, 7
        cand = np.stack([rng.permutation(ninter + nintra)[:n] for _ in range(nb)]).astype(np.uint8)
        cand_out = np.zeros((nb, n), mg.CAND_DTYPE); cand_out["flags"] = rng.integers(0, 4, (nb, n))
        cfl = np.zeros((nb, n), mg.CFL_DEC_DTYPE)
        cfl["uv_mode"] = rng.choice([0, 13], (nb, n)); cfl["cfl_alpha_idx"] = rng.integers(0, 256, (nb, n)) * (cfl["uv_mode"] == 13)
        cfl["cfl_alpha_signs"] = rng.integers(0, 8, (nb, n)) * (cfl["uv_mode"] == 13)
        blk = np.zeros(nb, mg.BLK_DTYPE); blk["skip_flag_context"] = rng.integers(0, 3, nb); blk["has_uv"] = np.arange(nb) % 3 != 1
        md = dict(bsize=bsize, nblocks=nb, n=n, ninter=ninter, nintra=nintra, modes=rng.permutation(13)[:nintra].astype(np.uint8), slice_is_intra=0,
                  full_loop_escape=1, rate=dev(rng.integers(0, 1 << 12, (nb, n, 2)).astype(np.uint32)), cand=dev(cand),
                  cand_out=dev(cand_out.view(np.uint8).reshape(nb, n, 16)), cfl=dev(cfl.view(np.uint8).reshape(nb, n, 32)),
                  blk=dev(blk.view(np.uint8).reshape(nb, 4)), rates=dev(gold["rates"]), pred=[pl["pred"] for pl in planes],
                  inter_blk=index_tensor(nb, n, 16, 11, torch.uint8))
        md["lambda"] = LAMBDA
        out.append(dict(md=md, planes=planes, sizes=sizes, host=dict(cand=cand, cand_out=cand_out, cfl=cfl, blk=blk, modes=md["modes"], rate=md["rate"].cpu().numpy().view(np.uint32))))
    return out


def md_outputs(base):
    """the decide's group with fresh poisoned outputs"""
    md, nb, n = dict(base["md"]), base["md"]["nblocks"], base["md"]["n"]
    md["decision"], md["full_cost"] = poison.tensor((nb, 72), torch.uint8, DEV), poison.tensor((nb, n), torch.int64, DEV)
    md["best_inter_blk"] = poison.tensor((nb, 16), torch.uint8, DEV)
    md["best_pred"] = [poison.tensor((nb, w * h), torch.uint8, DEV) for w, h, _ in base["sizes"]]
    md["best_qcoeff"] = [poison.tensor((nb, nc), torch.int32, DEV) for _, _, nc in base["sizes"]]
    md["best_dqcoeff"] = [poison.tensor((nb, nc), torch.int32, DEV) for _, _, nc in base["sizes"]]
    return md


def stage_outputs(base):
    """the arrays the stages hand to each other, poisoned: luma's record and best coefficients, chroma's dist / eob / bits / coefficients"""
    pairs = base["md"]["nblocks"] * base["md"]["n"]
    nc = [s[2] for s in base["sizes"]]
    luma = dict(decision=poison.tensor((pairs, 40), torch.uint8, DEV), best_qcoeff=poison.tensor((pairs, nc[0]), torch.int32, DEV),
                best_dqcoeff=poison.tensor((pairs, nc[0]), torch.int32, DEV))
    chroma = [dict(dist=poison.tensor((pairs, 1, 2), torch.int64, DEV), eob=poison.tensor((pairs, 1), torch.int16, DEV),
                   qcoeff=poison.tensor((pairs, 1, nc[p]), torch.int32, DEV), dqcoeff=poison.tensor((pairs, 1, nc[p]), torch.int32, DEV),
                   bits=poison.tensor((pairs, 1), torch.int64, DEV)) for p in (1, 2)]
    return luma, chroma


def search_group(base, md, luma_out=None, chroma_out=None):
    pl = base["planes"]
    g = dict(md=md, luma=dict(pl[0], **(luma_out or {})), cb=dict(pl[1], **{k: v for k, v in (chroma_out[0] if chroma_out else {}).items() if k != "bits"}),
             cr=dict(pl[2], **{k: v for k, v in (chroma_out[1] if chroma_out else {}).items() if k != "bits"}),
             txb_skip_ctx_c=[pl[1]["txb_skip_ctx"], pl[2]["txb_skip_ctx"]], dc_sign_ctx_c=[pl[1]["dc_sign_ctx"], pl[2]["dc_sign_ctx"]],
             coeff_cost_uv=pl[1]["coeff_cost"], eob_cost_uv=pl[1]["eob_cost"])
    if chroma_out:
        g["bits_c"] = [chroma_out[0]["bits"], chroma_out[1]["bits"]]
    return g


def qrows():
    q = svtlibs.quant_tables(8)
    return {k: np.ascontiguousarray(v[60]) for k, v in q.items()}, {k: np.ascontiguousarray(v[84]) for k, v in q.items()}


def same_md_outputs(a, b, what):
    for k in MD_OUT:
        assert torch.equal(a[k], b[k]), (what, k)
    for k in GATHERS:
        for p in range(3):
            assert torch.equal(a[k][p], b[k][p]), (what, k, p)


def test_search_frame_equals_the_stages_by_hand_and_the_restatement(dsp, gold):
    ql, qc = qrows()
    bases = search_inputs(gold)
    # by hand: the luma search, the chroma full loops and rates, the decide
    hand = []
    for b in bases:
        luma, chroma = stage_outputs(b)
        pl = b["planes"]
        hand.append(dict(luma=dict(pl[0], **luma), cb=dict(pl[1], **chroma[0]), cr=dict(pl[2], **chroma[1])))
    lumas = [h["luma"] for h in hand]
    scratch_tx = poison.tensor((max(dsp.tx_search_scratch_bytes(lumas), 16),), torch.uint8, DEV)
    assert dsp.tx_search_frame(lumas, ql, scratch_tx, 1) == 0, dsp.lib.svt_hip_last_error()
    chromas = [h[c] for h in hand for c in ("cb", "cr")]
    assert dsp.full_loop_frame(chromas, qc, 1) == 0, dsp.lib.svt_hip_last_error()
    assert dsp.coeff_rate_frame(chromas) == 0, dsp.lib.svt_hip_last_error()
    mds = []
    for b, h in zip(bases, hand):
        md = md_outputs(b)
        md.update(luma=h["luma"]["decision"], dist_cb=h["cb"]["dist"], dist_cr=h["cr"]["dist"], bits_cb=h["cb"]["bits"], bits_cr=h["cr"]["bits"],
                  eob_cb=h["cb"]["eob"], eob_cr=h["cr"]["eob"], qcoeff=[h["luma"]["best_qcoeff"], h["cb"]["qcoeff"], h["cr"]["qcoeff"]],
                  dqcoeff=[h["luma"]["best_dqcoeff"], h["cb"]["dqcoeff"], h["cr"]["dqcoeff"]])
        mds.append(md)
    assert dsp.md_decide_frame(mds) == 0, dsp.lib.svt_hip_last_error()
    # one call, the caller keeps every stage array
    kept_stage = [stage_outputs(b) for b in bases]
    kept = [search_group(b, md_outputs(b), lo, co) for b, (lo, co) in zip(bases, kept_stage)]
    need_kept = dsp.md_search_scratch_bytes(kept)
    assert need_kept == dsp.tx_search_scratch_bytes([g["luma"] for g in kept]) > 0        # only the luma search's own pieces
    s_kept = poison.tensor((need_kept,), torch.uint8, DEV)
    assert dsp.md_search_frame(kept, ql, qc, s_kept, 1) == 0, dsp.lib.svt_hip_last_error()
    # one call, everything in the scratch
    lean = [search_group(b, md_outputs(b)) for b in bases]
    need = dsp.md_search_scratch_bytes(lean)
    assert need > need_kept
    s_lean = poison.tensor((need,), torch.uint8, DEV)
    assert dsp.md_search_frame(lean, ql, qc, s_lean, 1) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()
    winners, kinds, coeffs = set(), set(), 0
    for b, h, md, gk, gl, (lo, co) in zip(bases, hand, mds, kept, lean, kept_stage):
        poison.assert_written([md[k] for k in MD_OUT] + [t for k in GATHERS for t in md[k]])
        same_md_outputs(md, gk["md"], ("kept", b["md"]["bsize"])); same_md_outputs(md, gl["md"], ("lean", b["md"]["bsize"]))
        for k in ("decision", "best_qcoeff", "best_dqcoeff"):
            assert torch.equal(h["luma"][k], lo[k]), k
        for p, c in enumerate(("cb", "cr")):
            for k in ("dist", "eob", "qcoeff", "dqcoeff", "bits"):
                assert torch.equal(h[c][k], co[p][k]), (c, k)
        # the restatement on the downloaded stage arrays
        nb, n = b["md"]["nblocks"], b["md"]["n"]
        host = b["host"]
        z = {"rates": gold["rates"], "c0_bsize": b["md"]["bsize"], "c0_n": n, "c0_ninter": b["md"]["ninter"], "c0_nintra": b["md"]["nintra"], "c0_lam": LAMBDA,
             "c0_slice_is_intra": 0, "c0_escape": 1, "c0_has_chroma": 1, "c0_has_cfl": 1, "c0_modes": host["modes"],
             "c0_luma": h["luma"]["decision"].cpu().numpy().reshape(nb, n, 40),
             "c0_cdist": np.stack([h[c]["dist"].cpu().numpy().view(np.uint64).reshape(nb, n, 2) for c in ("cb", "cr")]),
             "c0_cbits": np.stack([h[c]["bits"].cpu().numpy().view(np.uint64).reshape(nb, n) for c in ("cb", "cr")]),
             "c0_ceob": np.stack([h[c]["eob"].cpu().numpy().view(np.uint16).reshape(nb, n) for c in ("cb", "cr")]),
             "c0_rate": host["rate"], "c0_cand": host["cand"], "c0_cand_out": host["cand_out"].view(np.uint8).reshape(nb, n, 16),
             "c0_cfl": host["cfl"].view(np.uint8).reshape(nb, n, 32), "c0_blk": host["blk"].view(np.uint8).reshape(nb, 4)}
        dec, cost = mg.np_md_decide(z, 0)
        assert np.array_equal(md["decision"].cpu().numpy().view(mg.DEC_DTYPE).reshape(-1), dec), b["md"]["bsize"]
        assert np.array_equal(md["full_cost"].cpu().numpy().view(np.uint64), cost)
        for p, (w, hh, nc) in enumerate(b["sizes"]):
            assert np.array_equal(md["best_pred"][p].cpu().numpy(), mg.np_gather(dec, b["planes"][p]["pred"].cpu().numpy().reshape(nb, n, w * hh)))
            q = (h["luma"]["best_qcoeff"] if p == 0 else h[("cb", "cr")[p - 1]]["qcoeff"]).cpu().numpy().reshape(nb, n, nc)
            assert np.array_equal(md["best_qcoeff"][p].cpu().numpy(), mg.np_gather(dec, q, p))
        winners |= {int(s) for s in dec["slot"]}
        kinds |= {(int(i), int(m)) for i, m in zip(dec["is_intra"], dec["merge_flag"])}
        coeffs += int((dec["eob"] > 0).sum())
    assert len(winners) > 1 and len(kinds) > 1 and coeffs > 6               # the chain carried real coefficients and really chose


def test_search_frame_rejects_a_small_scratch_and_bad_stage_arguments(dsp, gold):
    ql, qc = qrows()
    bases = search_inputs(gold)[:2]
    lean = [search_group(b, md_outputs(b)) for b in bases]
    need = dsp.md_search_scratch_bytes(lean)
    scratch = poison.tensor((need,), torch.uint8, DEV)
    fill = poison.fill_value(torch.uint8)
    clean = lambda: bool((scratch == fill).all()) and all(untouched(g["md"]) for g in lean)
    assert dsp.md_search_frame(lean, ql, qc, scratch[:need - 16], 1) == INVALID
    assert dsp.md_search_frame(lean, ql, qc, scratch[8:], 1) == INVALID       # not 16-byte aligned (and short)
    assert dsp.md_search_frame(lean, ql, qc, None, 1) == INVALID
    assert dsp.md_search_frame(lean, ql, None, scratch, 1) == INVALID         # chroma without its rows
    assert dsp.md_search_frame(lean, ql, qc, scratch, 7) == INVALID           # flavour
    last = lean[1]
    sub = lambda key, **change: dict(last, **{key: dict(last[key], **change)})
    for name, bad in (("luma iscan", sub("luma", iscan=None)), ("luma cost table", sub("luma", coeff_cost=None)), ("luma without DCT_DCT", sub("luma", tx_types=[9], iscan=last["luma"]["iscan"])),
                      ("luma nblocks", sub("luma", nblocks=last["luma"]["nblocks"] - 1)), ("cb src", sub("cb", src=None)), ("cr two types", sub("cr", tx_types=[0, 9])),
                      ("chroma cost table", dict(last, coeff_cost_uv=None)), ("chroma context", dict(last, txb_skip_ctx_c=[last["txb_skip_ctx_c"][0], None])),
                      ("md decision", sub("md", decision=None)), ("md bsize", sub("md", bsize=13)), ("md rates", sub("md", rates=None)),
                      ("md gather misaligned", sub("md", best_pred=[last["md"]["best_pred"][0].reshape(-1)[8:]] + last["md"]["best_pred"][1:]))):
        assert dsp.md_search_frame([lean[0], bad], ql, qc, scratch, 1) == INVALID, name
    torch.cuda.synchronize()
    assert clean()
    assert dsp.md_search_frame(lean, ql, qc, scratch, 1) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()
    assert not clean()
