"""GPU: svt_hip_tx_decide_frame (RD cost, best transform type and the winner's coefficients per block) against the fixture
(tests/golden/tx_decide.npz: the reference's av1_tu_calc_cost_luma per pair, the generator's loop glue) and its numpy restatement, and
svt_hip_tx_search_frame (full loop -> coefficient rate -> decide in one call) against the three calls enqueued by hand."""
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
GOLD = os.path.join(ROOT, "tests", "golden", "tx_decide.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_coeff_rate as mgc  # noqa: E402
import make_golden_tx_decide as mg  # noqa: E402

INVALID = -2
OUTPUTS = ("decision", "best_qcoeff", "best_dqcoeff")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint64, np.uint16):                                     # torch has the signed types
        a = a.view(np.int64 if a.dtype == np.uint64 else np.int16)
    return torch.from_numpy(a).to(DEV)


def ncoeff(s):
    return min(TX_W[s], 32) * min(TX_H[s], 32)


def coeff_tensor(n, T, nc, salt):
    """int32 [n, T, nc] on the device, every entry a function of its indices (never 0, never the poison pattern's low bytes alone)"""
    i = lambda k, shape: torch.arange(k, dtype=torch.int32, device=DEV).view(shape)
    return (i(n, (n, 1, 1)) * 4099 + i(T, (1, T, 1)) * 1031 + i(nc, (1, 1, nc)) + salt).contiguous()


def coeff_expected(dec, nc, salt):
    """what np_gather would take from coeff_tensor: the winner's row, zeros for a winner with eob 0 or no winner"""
    n = len(dec)
    w = dec["type_index"].astype(np.int64)
    out = (np.arange(n, dtype=np.int64)[:, None] * 4099 + w[:, None] * 1031 + np.arange(nc, dtype=np.int64)[None, :] + salt).astype(np.int32)
    out[(dec["eob"] == 0) | (dec["type_index"] == mg.NO_CANDIDATE)] = 0
    return out


def case_group(z, k, type_order=None, blocks=None, want_q=True, want_dq=True):
    """(group dict, expected dict) of one fixture case: blocks (indices into the case's, default all) x types (default the case's order).
    In the case's own order the expected records are the fixture's; in another order the restatement's (a tie goes to the earlier type)."""
    s, ftypes, lam = int(z[f"c{k}_size"]), [int(t) for t in z[f"c{k}_types"]], int(z[f"c{k}_lam"])
    types = ftypes if type_order is None else list(type_order)
    perm = [ftypes.index(t) for t in types]
    blocks = np.arange(mg.NBLOCKS) if blocks is None else np.asarray(blocks)
    dist, eob, bits = z[f"c{k}_dist"][blocks][:, perm], z[f"c{k}_eob"][blocks][:, perm], z[f"c{k}_bits"][blocks][:, perm]
    dec = mg.decisions(z, k)[blocks] if type_order is None else mg.np_tx_decide(dist, eob, bits, types, lam)[0]
    n, T, nc = len(blocks), len(types), ncoeff(s)
    g = dict(tx_size=s, tx_types=types, nblocks=n, dist=dev(dist), eob=dev(eob), bits=dev(bits))
    g["lambda"] = lam
    g["decision"] = poison.tensor((n, 40), torch.uint8, DEV)
    want = dict(decision=dec)
    for key, on, salt in (("qcoeff", want_q, 7 + k), ("dqcoeff", want_dq, 900001 + k)):
        if on:
            g[key] = coeff_tensor(n, T, nc, salt)
            g["best_" + key] = poison.tensor((n, nc), torch.int32, DEV)
            want["best_" + key] = coeff_expected(dec, nc, salt)
    return g, want


def run(dsp, groups):
    rc = dsp.tx_decide_frame(groups)
    torch.cuda.synchronize()
    assert rc == 0, dsp.lib.svt_hip_last_error()


def check(groups, wants):
    for g, w in zip(groups, wants):
        got = g["decision"].cpu().numpy().view(mg.DEC_DTYPE).reshape(-1)
        bad = np.flatnonzero(got != w["decision"])
        assert bad.size == 0, (g["tx_size"], g["tx_types"], bad[:8].tolist(), got[bad[0]], w["decision"][bad[0]])
        for key in ("best_qcoeff", "best_dqcoeff"):
            if key in w:
                out = g[key].cpu().numpy()
                bad = np.argwhere(out != w[key])
                assert bad.size == 0, (g["tx_size"], key, bad[:8].tolist(), out[tuple(bad[0])], w[key][tuple(bad[0])])


def test_golden_fixture_all_cases_in_one_call(dsp, gold):
    """every fixture case bit for bit: the 19 sizes and the two lists without DCT_DCT as groups of one call, then each again with its types
    reversed and its blocks repeated in another order (131 blocks: a last wave-unit that is not full; 42 groups: two launches)"""
    groups, wants = [], []
    for k in range(mg.NCASES):
        g, w = case_group(gold, k)
        groups.append(g); wants.append(w)
    for k in range(mg.NCASES):
        types = [int(t) for t in gold[f"c{k}_types"]][::-1]
        g, w = case_group(gold, k, types, (np.arange(131) * 7) % mg.NBLOCKS)
        groups.append(g); wants.append(w)
    run(dsp, groups)
    check(groups, wants)
    none = sum(int((w["decision"]["type_index"] == mg.NO_CANDIDATE).sum()) for w in wants)
    zero = sum(int(((w["decision"]["eob"] == 0) & (w["decision"]["type_index"] != mg.NO_CANDIDATE)).sum()) for w in wants)
    assert none > 0 and zero > 0                                            # both zero-fill paths of the gather ran


def test_two_larger_groups(dsp, gold):
    """4x4 with 70 001 blocks of 16 types (274 workgroups, the last wave-unit ragged) and 32x32 with 1 037 blocks (2 blocks per wave-unit:
    130 workgroups, a last unit of one block), the fixture's blocks repeated"""
    groups, wants = [], []
    for k, n, dq in ((0, 70001, False), (3, 1037, True)):
        g, w = case_group(gold, k, None, (np.arange(n) * 11) % mg.NBLOCKS, want_dq=dq)
        groups.append(g); wants.append(w)
    run(dsp, groups)
    check(groups, wants)


@pytest.mark.parametrize("k,t,b", [(0, 0, 0), (3, 9, 4), (8, 10, 1), (4, 0, 6), (20, 9, 6)])
def test_single_group_of_one_block_and_one_type(dsp, gold, k, t, b):
    g, w = case_group(gold, k, [t], [b])
    run(dsp, [g])
    check([g], [w])


def test_empty_groups_and_no_groups(dsp, gold):
    g, w = case_group(gold, 7)
    empty = dict(tx_size=2, tx_types=[0, 9], nblocks=0)
    run(dsp, [empty, g, empty])
    check([g], [w])
    run(dsp, [])


def test_gather_with_both_arrays_one_or_none(dsp, gold):
    """d_best_qcoeff and d_best_dqcoeff are independent; a coefficient input without its output is read by nobody; winners with eob 0
    give zeros; the guards around every output (the fixture checks them) see any entry beyond [nblocks][NC]"""
    groups, wants = [], []
    for k, q, dq in ((1, True, True), (5, True, False), (5, False, False), (13, True, True), (10, True, False), (19, True, True)):
        g, w = case_group(gold, k, None, np.arange(37), want_q=q, want_dq=dq)
        groups.append(g); wants.append(w)
    g, w = case_group(gold, 6)                                              # inputs given, no output asked for
    del g["best_qcoeff"], g["best_dqcoeff"], w["best_qcoeff"], w["best_dqcoeff"]
    groups.append(g); wants.append(w)
    run(dsp, groups)
    check(groups, wants)
    d = wants[0]["decision"]
    zero = (d["eob"] == 0) & (d["type_index"] != mg.NO_CANDIDATE)
    assert zero.any() and not wants[0]["best_qcoeff"][zero].any() and wants[0]["best_qcoeff"][~zero].all()


def test_wrapper_allocates_the_missing_outputs(dsp, gold):
    """tx_decide allocates decision and one best array per coefficient input given (through t.empty: poisoned and fenced here)"""
    g, w = case_group(gold, 2)
    dec, bq, bdq = dsp.tx_decide(g["dist"], g["eob"], g["bits"], g["tx_size"], g["tx_types"], g["lambda"], qcoeff=g["qcoeff"], dqcoeff=g["dqcoeff"])
    torch.cuda.synchronize()
    check([dict(g, decision=dec, best_qcoeff=bq, best_dqcoeff=bdq)], [w])
    dec, bq, bdq = dsp.tx_decide(g["dist"], g["eob"], g["bits"], g["tx_size"], g["tx_types"], g["lambda"])
    torch.cuda.synchronize()
    assert bq is None and bdq is None
    check([dict(g, decision=dec)], [dict(decision=w["decision"])])


def test_graph_capture_and_two_replays(dsp, gold):
    groups, wants = [], []
    for k in (1, 13, 10, 12, 19):
        g, w = case_group(gold, k)
        groups.append(g); wants.append(w)
    arr = dsp.make_tx_decide_groups(groups)
    run(dsp, arr)                                                         # warm: nothing is created inside the capture
    check(groups, wants)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert dsp.tx_decide_frame(arr) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for g in groups:
            for key in OUTPUTS:
                g[key].view(torch.uint8).fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        check(groups, wants)


def untouched(g):
    fill = poison.fill_value(torch.uint8)
    return all(bool((g[key].view(torch.uint8) == fill).all()) for key in OUTPUTS if g.get(key) is not None)


def invalid_cases(g):
    """(name, changes to a valid group) that svt_hip_tx_decide_frame must reject"""
    off = lambda k, n: g[k].reshape(-1).view(torch.uint8)[n:]              # the same buffer, n bytes in
    return [("tx_size -1", dict(tx_size=-1)), ("tx_size 19", dict(tx_size=19)), ("ntypes 0", dict(ntypes=0)), ("ntypes 17", dict(ntypes=17)),
            ("type not defined for the size", dict(tx_size=3, tx_types=[0, 1])), ("type 16", dict(tx_types=[0, 16])),
            ("duplicate type", dict(tx_types=[0, 0])), ("nblocks * ntypes too large", dict(nblocks=0x40000000)),
            ("NULL dist", dict(dist=None)), ("NULL eob", dict(eob=None)), ("NULL bits", dict(bits=None)), ("NULL decision", dict(decision=None)),
            ("best_qcoeff without qcoeff", dict(qcoeff=None)), ("best_dqcoeff without dqcoeff", dict(dqcoeff=None)),
            ("best_qcoeff is qcoeff", dict(best_qcoeff=g["qcoeff"])), ("best_dqcoeff is dqcoeff", dict(best_dqcoeff=g["dqcoeff"])),
            ("dist 8-byte aligned", dict(dist=off("dist", 8))), ("qcoeff 8-byte aligned", dict(qcoeff=off("qcoeff", 8))),
            ("dqcoeff 4-byte aligned", dict(dqcoeff=off("dqcoeff", 4))), ("best_qcoeff 8-byte aligned", dict(best_qcoeff=off("best_qcoeff", 8))),
            ("best_dqcoeff 4-byte aligned", dict(best_dqcoeff=off("best_dqcoeff", 4))), ("bits 4-byte aligned", dict(bits=off("bits", 4))),
            ("decision 4-byte aligned", dict(decision=off("decision", 4))), ("eob 1-byte aligned", dict(eob=off("eob", 1)))]


def test_invalid_arguments_return_before_any_launch(dsp, gold):
    good, w = case_group(gold, 1, [0, 10])
    other, _ = case_group(gold, 2)
    for name, change in invalid_cases(good):
        bad = dict(good, **change)
        for order in ([other, bad], [bad, other]):                       # the bad group last: nothing before it may have run
            arr = dsp.make_tx_decide_groups(order)                       # (the wrapper would allocate a missing "decision")
            assert dsp.tx_decide_frame(arr) == INVALID, name
            torch.cuda.synchronize()
            assert untouched(good) and untouched(other), name
    # an empty group's size and types are validated too
    for change in (dict(tx_size=19), dict(tx_types=[0, 0]), dict(tx_size=4, tx_types=[9])):
        arr = dsp.make_tx_decide_groups([other, dict(dict(tx_size=1, tx_types=[0], nblocks=0), **change)])
        assert dsp.tx_decide_frame(arr) == INVALID, change
    assert dsp.lib.svt_hip_tx_decide_frame(None, 1, None) == INVALID and dsp.lib.svt_hip_tx_decide_frame(None, -1, None) == INVALID
    torch.cuda.synchronize()
    assert untouched(other)
    run(dsp, [good])
    check([good], [w])


# ---- the whole search in one call ------------------------------------------------------------------------------------------------
SEARCH_SIZES = (0, 8, 3, 4)                                              # 4x4, 16x8, 32x32, 64x64
LAMBDA = 29041


def search_inputs():
    """per size: a few blocks of a picture-like source with a near prediction, contexts, type bits and cost tables"""
    rng = np.random.default_rng(4127)
    out = []
    for s in SEARCH_SIZES:
        w, h, n = TX_W[s], TX_H[s], 8
        types = [t for t in range(16) if txfm_allowed(s, t)]
        src = rng.integers(0, 256, (n, h, w)).astype(np.uint8)
        pred = np.clip(src.astype(np.int32) + rng.integers(-12, 13, (n, h, w)) * (rng.random((n, 1, 1)) < 0.8), 0, 255).astype(np.uint8)
        cc, ec = mgc.tables_of(s)
        out.append(dict(tx_size=s, tx_types=types, nblocks=n, src=dev(src), pred=dev(pred), iscan=dev(np.stack([svtlibs.scan_tables(s, t)[1] for t in types])),
                        txb_skip_ctx=dev(rng.integers(0, 13, n).astype(np.uint8)), dc_sign_ctx=dev(rng.integers(0, 3, n).astype(np.uint8)),
                        type_bits=dev(rng.integers(0, 1 << 12, (n, len(types))).astype(np.int32)), coeff_cost=dev(cc), eob_cost=dev(ec)))
        out[-1]["lambda"] = LAMBDA
    return out


def with_outputs(base, per_type):
    """the group with fresh poisoned outputs; per_type: the caller keeps dist / eob / qcoeff / dqcoeff (and, for the calls by hand, bits)"""
    g = dict(base)
    n, T, nc = g["nblocks"], len(g["tx_types"]), ncoeff(g["tx_size"])
    g["decision"] = poison.tensor((n, 40), torch.uint8, DEV)
    g["best_qcoeff"], g["best_dqcoeff"] = poison.tensor((n, nc), torch.int32, DEV), poison.tensor((n, nc), torch.int32, DEV)
    if per_type:
        g["dist"], g["eob"] = poison.tensor((n, T, 2), torch.int64, DEV), poison.tensor((n, T), torch.int16, DEV)
        g["qcoeff"], g["dqcoeff"] = poison.tensor((n, T, nc), torch.int32, DEV), poison.tensor((n, T, nc), torch.int32, DEV)
        g["bits"] = poison.tensor((n, T), torch.int64, DEV)
    return g


def test_search_frame_equals_the_three_calls_and_the_restatement(dsp):
    qrow = {k: np.ascontiguousarray(v[60]) for k, v in svtlibs.quant_tables(8).items()}
    base = search_inputs()
    hand = [with_outputs(b, True) for b in base]
    assert dsp.full_loop_frame(hand, qrow, 1) == 0, dsp.lib.svt_hip_last_error()
    assert dsp.coeff_rate_frame(hand) == 0, dsp.lib.svt_hip_last_error()
    assert dsp.tx_decide_frame(hand) == 0, dsp.lib.svt_hip_last_error()
    kept = [with_outputs(b, True) for b in base]                          # one call, the caller keeps the per-type arrays
    need_kept = dsp.tx_search_scratch_bytes(kept)
    assert need_kept == sum((g["nblocks"] * len(g["tx_types"]) * 8 + 15) // 16 * 16 for g in kept)        # only the bits
    scratch_kept = poison.tensor((need_kept,), torch.uint8, DEV)
    assert dsp.tx_search_frame(kept, qrow, scratch_kept, 1) == 0, dsp.lib.svt_hip_last_error()
    lean = [with_outputs(b, False) for b in base]                         # one call, everything per-type in the scratch
    need = dsp.tx_search_scratch_bytes(lean)
    assert need > need_kept
    scratch = poison.tensor((need,), torch.uint8, DEV)
    assert dsp.tx_search_frame(lean, qrow, scratch, 1) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()
    poison.assert_written([[g[k] for k in ("dist", "eob", "qcoeff", "dqcoeff", "bits", "best_qcoeff", "best_dqcoeff")] for g in hand])
    winners, coeffs = set(), 0
    for gh, gk, gl in zip(hand, kept, lean):
        s, types, n = gh["tx_size"], gh["tx_types"], gh["nblocks"]
        for k in ("dist", "eob", "qcoeff", "dqcoeff"):
            assert torch.equal(gh[k], gk[k]), (s, k)
        for k in OUTPUTS:
            assert torch.equal(gh[k], gk[k]) and torch.equal(gh[k], gl[k]), (s, k)
        # the restatements on the downloaded per-type arrays
        q, dq = gh["qcoeff"].cpu().numpy(), gh["dqcoeff"].cpu().numpy()
        eob, dist = gh["eob"].cpu().numpy().view(np.uint16), gh["dist"].cpu().numpy().view(np.uint64)
        sk, dc, tb = gh["txb_skip_ctx"].cpu().numpy(), gh["dc_sign_ctx"].cpu().numpy(), gh["type_bits"].cpu().numpy()
        cc, ec = mgc.tables_of(s)
        bits = np.zeros(eob.shape, np.int64)
        for ti, t in enumerate(types):
            scan = mgc.scan_of(s, t)
            for b in range(n):
                bits[b, ti] = mgc.np_cost_coeffs_txb(q[b, ti], int(eob[b, ti]), s, t, int(sk[b]), int(dc[b]), cc, ec, scan) + (int(tb[b, ti]) if eob[b, ti] else 0)
        assert np.array_equal(gh["bits"].cpu().numpy(), bits), s
        dec, _ = mg.np_tx_decide(dist, eob, bits.view(np.uint64), types, LAMBDA)
        assert np.array_equal(gh["decision"].cpu().numpy().view(mg.DEC_DTYPE).reshape(-1), dec), s
        assert np.array_equal(gh["best_qcoeff"].cpu().numpy(), mg.np_gather(dec, q)) and np.array_equal(gh["best_dqcoeff"].cpu().numpy(), mg.np_gather(dec, dq)), s
        winners |= {int(t) for t in dec["tx_type"]}
        coeffs += int((dec["eob"] > 1).sum())
    assert len(winners) > 2 and coeffs > 8                                 # the chain carried real coefficients and really chose


def test_search_frame_without_dqcoeff_anywhere(dsp):
    """dqcoeff neither supplied nor asked for: nothing is carved for it, the full loop runs without d_dqcoeff and the decide call without
    d_best_dqcoeff; the record and best_qcoeff equal the search that does carry dqcoeff"""
    qrow = {k: np.ascontiguousarray(v[60]) for k, v in svtlibs.quant_tables(8).items()}
    base = search_inputs()
    full = [with_outputs(b, False) for b in base]
    lean = [with_outputs(b, False) for b in base]
    for g in lean:
        del g["best_dqcoeff"]
    need_full, need = dsp.tx_search_scratch_bytes(full), dsp.tx_search_scratch_bytes(lean)
    assert need == need_full - sum(g["nblocks"] * len(g["tx_types"]) * ncoeff(g["tx_size"]) * 4 for g in lean)
    s_full, s_lean = poison.tensor((need_full,), torch.uint8, DEV), poison.tensor((need,), torch.uint8, DEV)
    assert dsp.tx_search_frame(full, qrow, s_full, 1) == 0, dsp.lib.svt_hip_last_error()
    assert dsp.tx_search_frame(lean, qrow, s_lean, 1) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()
    poison.assert_written([g["best_qcoeff"] for g in lean])
    for gf, gl in zip(full, lean):
        assert torch.equal(gf["decision"], gl["decision"]) and torch.equal(gf["best_qcoeff"], gl["best_qcoeff"]), gf["tx_size"]
        assert bool((gl["decision"].view(torch.int64) != poison.fill_value(torch.int64)).all())


def test_search_frame_rejects_a_small_scratch_and_bad_stage_arguments(dsp):
    qrow = {k: np.ascontiguousarray(v[60]) for k, v in svtlibs.quant_tables(8).items()}
    base = search_inputs()[:2]
    lean = [with_outputs(b, False) for b in base]
    need = dsp.tx_search_scratch_bytes(lean)
    scratch = poison.tensor((need,), torch.uint8, DEV)
    fill = poison.fill_value(torch.uint8)
    clean = lambda: bool((scratch == fill).all()) and all(untouched(g) for g in lean)
    assert dsp.tx_search_frame(lean, qrow, scratch[:need - 16], 1) == INVALID
    assert dsp.tx_search_frame(lean, qrow, scratch[8:], 1) == INVALID       # not 16-byte aligned (and short)
    assert dsp.tx_search_frame(lean, qrow, None, 1) == INVALID
    # a bad argument of each stage, in the last group: full loop (iscan), coefficient rate (cost table), decide (decision)
    for change in (dict(iscan=None), dict(coeff_cost=None), dict(txb_skip_ctx=None), dict(decision=None), dict(best_qcoeff=lean[1]["best_qcoeff"].reshape(-1).view(torch.uint8)[8:])):
        assert dsp.tx_search_frame([lean[0], dict(lean[1], **change)], qrow, scratch, 1) == INVALID, list(change)
    assert dsp.tx_search_frame(lean, qrow, scratch, 7) == INVALID           # flavour
    torch.cuda.synchronize()
    assert clean()
    assert dsp.tx_search_frame(lean, qrow, scratch, 1) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()
    assert not clean()
