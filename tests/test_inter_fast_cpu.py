"""CPU: tests/golden/inter_fast.npz (the inter fast pick and search, make_golden_inter_fast.py) against a second, independent numpy
restatement kept here; the device tables of csrc/kernel_inter_fast_pick.h against the fixture's recorded tables; the ctypes mirrors'
sizes against the sizeofs the host program prints; and, where oracle/_ref is built, the generator run again with its leaf comparisons."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_fast_pick as FP  # noqa: E402
import make_golden_inter_fast as G  # noqa: E402
import make_golden_inter_pred as IP  # noqa: E402

PKG = os.path.join(ROOT, "cidana-svt-av1_amd")
KERNEL = os.path.join(PKG, "csrc", "kernel_inter_fast_pick.h")
OUTPUTS = ("cand", "sorted", "cost", "rate", "ref_fast_cost", "all_cost", "blk_out", "cand_out", "src_xy_out")


@pytest.fixture(scope="module")
def z():
    return np.load(G.OUT)


@pytest.fixture(scope="module")
def mv_cost(z):
    t = G.make_mv_cost()
    assert zlib.crc32(t.tobytes()) == int(z["mv_cost_crc"][0])
    return t


def case_of(z, kind, i):
    """(params, arrays) of pick group i or search group i"""
    keys, rows = (G.PICK_KEYS, z["pick_params"]) if kind == "pick" else (G.SEARCH_KEYS, z["search_params"])
    P = G.params_of(keys, rows[i])
    A = {k[len(f"{kind}_{i}_"):]: z[k] for k in z.files if k.startswith(f"{kind}_{i}_")}
    A["rates"] = A["rates"] if "rates" in A else z["rate_sets"][P["rate_set"]]
    return P, A


# ---- the second restatement: numpy over all candidates of a group at once ------------------------------------------------------------------
def np_costs(P, A, mv_cost):
    """-> cost uint64 [nb, ni], fast_luma_rate uint32 [nb, ni]"""
    R = G.unpack_rates(A["rates"])
    b = A["blk"].copy().view(G.BLK_DTYPE)[..., 0]
    c = A["cand_in"].copy().view(G.CAND_DTYPE)[..., 0]
    x = A["ctx"].copy().view(G.CTX_DTYPE)[..., 0][:, None]                    # [nb, 1]
    mode, rft = c["pred_mode"].astype(np.int64), c["ref_frame_type"].astype(np.int64)
    comp = b["pred_direction"] == 2
    rfmap = np.array([(t, -1) for t in range(8)] + list(G.REF_FRAME_MAP), np.int64)
    rf0, rf1 = rfmap[rft, 0], rfmap[rft, 1]
    T = lambda name: R[name].astype(np.int64)
    bits = np.zeros(mode.shape, np.int64)
    bw, bh = G.BSIZE_WH[P["bsize"]]
    if P["reference_mode_select"] and min(bw, bh) >= 8:
        bits += T("compInterFacBits")[x["reference_mode_context"], comp.astype(np.int64)]
    # compound reference bits
    cr, cb = T("compRefFacBits"), T("compBwdRefFacBits")
    fwd_hi = (rf0 == 3) | (rf0 == 4)
    cbits = T("compRefTypeFacBits")[x["compoud_reference_type_context"], 1] + cr[x["comp_ref_p"], 0, fwd_hi.astype(np.int64)]
    cbits = cbits + np.where(fwd_hi, cr[x["comp_ref_p2"], 2, (rf0 == 4).astype(np.int64)], cr[x["comp_ref_p1"], 1, (rf0 == 2).astype(np.int64)])
    cbits = cbits + cb[x["comp_bwdref_p"], 0, (rf1 == 7).astype(np.int64)] + np.where(rf1 == 7, 0, cb[x["comp_bwdref_p1"], 1, (rf1 == 6).astype(np.int64)])
    # single reference bits: a decision tree over ref_frame_type
    sr, sp = T("singleRefFacBits"), x["single_ref_p"].astype(np.int64)          # [nb, 1, 6]
    S = lambda node, bit: sr[sp[..., node], node, np.broadcast_to(bit, mode.shape).astype(np.int64)]
    bwd = (rft >= 5) & (rft <= 7)
    sbits = S(0, bwd) + np.where(bwd, S(1, rft == 7) + np.where(rft == 7, 0, S(5, rft == 6)),
                                 S(2, (rft == 3) | (rft == 4)) + np.where((rft == 3) | (rft == 4), S(4, rft != 3), S(3, rft != 1)))
    bits += np.where(comp, cbits, sbits)
    # mode context and mode bits
    mc = c["mode_ctx"].astype(np.int64) & 0xFFFFFFFF
    cmap = np.array(G.COMPOUND_MODE_CTX_MAP_2, np.int64)
    ctx_c = cmap[np.minimum(((mc >> 4) & 15) >> 1, 2), np.minimum(mc & 7, 4)]
    mctx = np.where(rf1 > 0, ctx_c, mc)
    single = (T("newMvModeFacBits")[np.minimum(mctx & 7, 5), (mode != 16).astype(np.int64)] +
              np.where(mode != 16, T("zeroMvModeFacBits")[(mctx >> 3) & 1, (mode != 15).astype(np.int64)], 0) +
              np.where((mode != 16) & (mode != 15), T("refMvModeFacBits")[np.minimum((mctx >> 4) & 15, 5), (mode != 13).astype(np.int64)], 0))
    bits += np.where(comp, T("interCompoundModeFacBits")[np.minimum(mctx, 7), np.clip(mode - 17, 0, 7)], single)
    # DRL: which of the indices are coded
    cnt, di, dctx = c["ref_mv_count"].astype(np.int64), c["drl_index"].astype(np.int64), c["drl_ctx"].astype(np.int64)
    drl = T("drlModeFacBits")
    for modes, first in (((16, 24), 0), ((14, 18, 21, 22), 1)):
        active = np.isin(mode, modes)
        for idx in (first, first + 1):
            coded = active & (cnt > idx + 1)
            bits += np.where(coded, drl[np.minimum((dctx >> (2 * idx)) & 3, 2), (di != idx - first).astype(np.int64)], 0)
            active = active & ~(coded & (di == idx - first))
    # MV rate
    mvc = mv_cost.astype(np.int64)
    joint = T("nmv_vec_cost")

    def mv_bits(l):
        row = b["mv"][..., l, 1].astype(np.int64) - c["pred_mv"][..., l, 1]
        col = b["mv"][..., l, 0].astype(np.int64) - c["pred_mv"][..., l, 0]
        assert np.abs(row).max() <= G.MV_MAX and np.abs(col).max() <= G.MV_MAX
        cost = joint[2 * (row != 0) + (col != 0)] + mvc[0, G.MV_MAX + row] + mvc[1, G.MV_MAX + col]
        return (cost * 108 + 64) >> 7
    has_new = np.isin(mode, (16, 19, 20, 21, 22, 24))
    use0 = np.where(comp, np.isin(mode, (24, 20, 22, 16)), b["pred_direction"] == 0)
    use1 = np.where(comp, np.isin(mode, (24, 19, 21)), b["pred_direction"] != 0)
    bits += np.where(has_new & use0, mv_bits(0), 0) + np.where(has_new & use1, mv_bits(1), 0)
    # motion mode
    flags = c["flags"].astype(np.int64)
    allowed, mm = (flags >> 3) & 3, (flags >> 1) & 3
    if P["switchable_motion_mode"]:
        bits += np.where((mode <= 16) & (allowed == 1), T("motionModeFacBits1")[P["bsize"], np.minimum(mm, 1)], 0)
        bits += np.where((mode <= 16) & (allowed >= 2), T("motionModeFacBits")[P["bsize"], np.minimum(mm, 2)], 0)
    lr = (bits + T("skipModeFacBits")[x["skip_flag_context"], 0] + T("intraInterFacBits")[x["is_inter_ctx"], 1]) & 0xFFFFFFFF
    luma = A["dist"].astype(np.uint64)
    chroma = (A["dist_cb"].astype(np.uint64) + A["dist_cr"].astype(np.uint64)) if "dist_cb" in A else np.zeros_like(luma)
    if P["metric"] == G.SSD:
        r1, d1 = FP.np_model_rd(luma, G.NUM_PELS_LOG2[P["bsize"]], P["ac_dequant_q3"])
        r2, d2 = FP.np_model_rd(chroma, G.NUM_PELS_LOG2[P["bsize_uv"]], P["ac_dequant_q3"])
        rate = (((lr + r1.astype(np.int64)) & 0xFFFFFFFF) + r2.astype(np.int64)) & 0xFFFFFFFF
        total = d1.astype(np.uint64) + d2.astype(np.uint64)
    else:
        rate, total = lr, luma + chroma
    skip1 = np.broadcast_to(T("skipModeFacBits")[x["skip_flag_context"], 1], mode.shape)
    rate = np.where(((flags & 1) == 1) & (skip1 < rate), skip1, rate)
    cost = ((rate.astype(np.uint64) * np.uint64(P["lambda"]) + np.uint64(256)) >> np.uint64(9)) + total * np.uint64(128)
    return cost, lr.astype(np.uint32)


def np_pick_block(costs, ninter, nfl):
    """walk, the inter-before-intra pass in closed form, order -> cand[n], sorted slots[n], ref_fast_cost"""
    nc = len(costs)
    n = min(nfl, nc)
    bufs = [nc - 1 - b for b in range(min(nc, n + 1))]                        # the last entries fill the buffers in order
    empty = None
    if nc > n:
        for c in range(nc - n - 2, -1, -1):                                   # the first buffer of the largest cost is overwritten
            held = [costs[k] for k in bufs]
            bufs[held.index(max(held))] = c
        held = [costs[k] for k in bufs]
        empty = held.index(max(held))
    bcost = [G.MAX_CU_COST if i == empty else costs[k] for i, k in enumerate(bufs)]
    order = [i for i in range(len(bufs)) if i != empty]                       # buffers by position
    p = [i for i, bi in enumerate(order) if bufs[bi] < ninter]                # positions of the inter entries
    for k, pk in enumerate(p):                                                # exchange k and p_k, k ascending
        order[k], order[pk] = order[pk], order[k]
    ref = min([G.MAX_MODE_COST] + bcost[:n])
    srt = list(order)
    for i in range(n - 1):
        for j in range(i + 1, n):
            if bcost[j] < bcost[i]:
                srt[i], srt[j] = srt[j], srt[i]
    return [bufs[bi] for bi in order], [order.index(bi) for bi in srt], ref


def np_pick(P, A, mv_cost):
    cost, lr = np_costs(P, A, mv_cost)
    nb, ni = cost.shape
    na = P["nintra"]
    n = min(P["nfl"], ni + na)
    blk, cand = A["blk"].copy().view(G.BLK_DTYPE)[..., 0], A["cand_in"].copy().view(G.CAND_DTYPE)[..., 0]
    out = dict(all_cost=cost, cand=np.zeros((nb, n), np.uint8), sorted=np.zeros((nb, n), np.uint8), cost=np.zeros((nb, n), np.uint64),
               rate=np.zeros((nb, n, 2), np.uint32), ref_fast_cost=np.zeros(nb, np.uint64), blk_out=np.zeros((nb, n), G.BLK_DTYPE),
               cand_out=np.zeros((nb, n), G.CAND_DTYPE), src_xy_out=np.zeros((nb, n), np.uint32))
    for i in range(nb):
        costs = [int(v) for v in cost[i]] + ([int(v) for v in A["intra_cost"][i]] if na else [])
        cd, sl, ref = np_pick_block(costs, ni, P["nfl"])
        out["cand"][i], out["sorted"][i], out["ref_fast_cost"][i] = cd, sl, ref
        out["src_xy_out"][i] = int(blk[i, 0]["x"]) | int(blk[i, 0]["y"]) << 16
        for s, k in enumerate(cd):
            out["cost"][i, s] = costs[k]
            if k < ni:
                out["rate"][i, s, 0], out["blk_out"][i, s], out["cand_out"][i, s] = lr[i, k], blk[i, k], cand[i, k]
            else:
                out["blk_out"][i, s]["x"], out["blk_out"][i, s]["y"] = blk[i, 0]["x"], blk[i, 0]["y"]
                if "intra_rate" in A:
                    out["rate"][i, s] = A["intra_rate"][i, k - ni]
    return out


def as_bytes(a):
    return a.view(np.uint8).reshape(a.shape + (16,)) if a.dtype.itemsize == 16 else a


@pytest.mark.parametrize("kind,i", [("pick", i) for i in range(len(G.PICK_GROUPS))] + [("search", i) for i in range(len(G.SEARCH_GROUPS))])
def test_fixture_against_second_restatement(z, mv_cost, kind, i):
    """every recorded output of every group equals the vectorised restatement (cost) and the closed-form one (walk, swap pass, order)"""
    P, A = case_of(z, kind, i)
    out = np_pick(P, A, mv_cost)
    for name in OUTPUTS:
        got, want = as_bytes(out[name]), A["out_" + name]
        assert got.shape == want.shape and (got.astype(np.uint64) == want.astype(np.uint64)).all(), (kind, i, name)


def test_fixture_records_its_coverage(z):
    """the cases the generator asserts on regeneration, as the stored counts show them"""
    assert z["coverage_modes"].tolist() == list(range(13, 25))
    assert set(range(1, 8)) <= set(z["coverage_types"].tolist()) and (z["coverage_types"] >= 8).sum() >= 6
    assert {(c, d) for c in range(5) for d in range(3)} <= set(map(tuple, z["coverage_drl"].tolist()))
    fired, idle, all_intra, iii = z["coverage_walk"].tolist()
    assert fired > 0 and idle > 0 and all_intra > 0 and iii > 0
    ncost, over, npairs, outside = z["domain"].tolist()
    assert ncost > 0 and over == 0 and npairs > 0 and outside == 0
    shapes = {tuple(r[:3]) for r in z["pick_params"].tolist()}
    assert {(1, 0, 1), (2, 0, 1), (3, 0, 3), (4, 0, 3), (13, 0, 12), (64, 0, 40), (5, 3, 3), (5, 3, 12), (40, 24, 40), (1, 63, 2)} <= shapes
    assert z["planes_crc"].tolist() == [IP.planes_crc(IP.planes_of(bd, "random")) for bd in (8, 10)]


def test_swap_pass_closed_form():
    """the :458-469 pass on every type pattern up to nine entries: the literal loops against "exchange k and p_k"; [A, B, c] -> [c, B, A]"""
    assert G.sort_mixed([3, 2, 1], [True, True, False], 3)[0] == [2, 1, 0]
    for n in range(1, 10):
        for bits in range(1 << n):
            intra = [bool(bits >> i & 1) for i in range(n)]
            lit = G.sort_mixed(list(range(100, 100 + n)), intra, n)[0]
            order = list(range(n))
            for k, pk in enumerate([i for i in range(n) if not intra[i]]):
                order[k], order[pk] = order[pk], order[k]
            assert lit == order, (intra, lit, order)


def test_swap_pass_as_the_kernel_states_it():
    """the form inter_pick_kernel runs, in Python: M the positions of the inter entries, K = |M|; an inter entry goes to its rank in M,
    destination d >= K takes the entry found by following m -> |M below m| from d until m leaves M.  Every pattern up to twelve
    entries against the literal loops; every chain ends within n steps"""
    popc = lambda v: bin(v).count("1")
    for n in range(1, 13):
        for bits in range(1 << n):
            intra = [bool(bits >> i & 1) for i in range(n)]
            M = sum((0 if intra[i] else 1) << i for i in range(n))
            K = popc(M)
            dest = list(range(n))
            for d in range(K, n):
                m, steps = d, 0
                while (M >> m) & 1:
                    m, steps = popc(M & ((1 << m) - 1)), steps + 1
                    assert steps <= n
                dest[m] = d
            out = [None] * n
            for pos in range(n):
                out[dest[pos] if intra[pos] else popc(M & ((1 << pos) - 1))] = pos
            assert out == G.sort_mixed(list(range(100, 100 + n)), intra, n)[0], intra


def test_device_tables_match_fixture(z):
    """kIfpRefFrameMap, kIfpCompCtxMap and the table offsets parsed from the kernel header against what the fixture recorded"""
    src = open(KERNEL).read()
    m = re.search(r"kIfpRefFrameMap\[21\] = \{([^}]*)\}", src)
    dev = [int(t, 16) for t in re.findall(r"0x[0-9a-fA-F]+", m.group(1))]
    rec = z["ref_frame_map"]
    assert len(dev) == 21 and [(v & 15, v >> 4) for v in dev] == [tuple(r) for r in rec[8:29].tolist()]
    assert [tuple(r) for r in rec[1:8].tolist()] == [(t, -1) for t in range(1, 8)]
    m = re.search(r"kIfpCompCtxMap\[3\] = \{([^}]*)\}", src)
    rows = []
    for row in m.group(1).split(","):
        terms = [t.strip() for t in row.split("|")]
        rows.append([int(t.split("<<")[0]) for t in terms])
    assert rows == z["compound_mode_ctx_map_2"].tolist()
    # the offsets of svt_hip_inter_fast_rates as words
    names = ("IFP_SKIP", "IFP_NEWMV", "IFP_ZEROMV", "IFP_REFMV", "IFP_DRL", "IFP_COMPMODE", "IFP_SINGLE", "IFP_CRT", "IFP_CREF", "IFP_CBWD",
             "IFP_CINTER", "IFP_MM", "IFP_MM1", "IFP_II", "IFP_JOINT", "IFP_RATE_WORDS")
    decl = re.search(r"constexpr int IFP_SKIP = 0,(.*?);", src, re.S).group(0)
    order = re.findall(r"(IFP_[A-Z0-9_]+) =", decl)
    assert tuple(order) == names
    sizes = [int(np.prod(s)) for _, s in G.RATE_TABLES]
    dims = re.findall(r"= IFP_[A-Z0-9]+ \+ ([0-9 *]+)[,;]", decl)
    assert [int(np.prod([int(v) for v in d.split("*")])) for d in dims] == sizes
    assert G.RATE_WORDS == sum(sizes) == 383


def test_ctypes_mirrors_match_sizeof(tmp_path):
    """the Python mirrors of the new structs against the sizeofs of the C declarations, printed by the stand-alone host program"""
    import ctypes
    import __graft_entry__ as ge
    pkg = ge.load_package()
    exe = str(tmp_path / "inter_fast_plan_host")
    pr = subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "c", "inter_fast_plan_host.cpp"), os.path.join(PKG, "csrc", "host_tables.cpp"),
                         os.path.join(PKG, "csrc", "host_err.cpp"), "-o", exe], capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr[-4000:]
    out = subprocess.run([exe, "sizes"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    sizes = {k: int(v) for k, v in (line.split() for line in out.stdout.strip().splitlines())}
    mirrors = dict(svt_hip_inter_blk=pkg.InterBlk, svt_hip_inter_cand=pkg.InterCand, svt_hip_inter_fast_blk=pkg.InterFastBlk,
                   svt_hip_inter_fast_rates=pkg.InterFastRates, svt_hip_inter_fast_pick_group=pkg.InterFastPickGroup,
                   svt_hip_inter_fast_search_group=pkg.InterFastSearchGroup, svt_hip_inter_pred_group=pkg.InterPredGroup)
    assert set(sizes) == set(mirrors)
    for name, cls in mirrors.items():
        assert ctypes.sizeof(cls) == sizes[name], name
    assert pkg.inter_cand_dtype().itemsize == 16 and pkg.inter_fast_blk_dtype().itemsize == 16
    assert pkg.inter_cand_dtype() == G.CAND_DTYPE and pkg.inter_fast_blk_dtype() == G.CTX_DTYPE
    assert pkg.INTER_FAST_RATE_TABLES == G.RATE_TABLES and pkg.INTER_FAST_RATE_WORDS * 4 == sizes["svt_hip_inter_fast_rates"]
    assert pkg.MV_VALS == G.MV_VALS and pkg.SvtHipDsp.MAX_NFL == 40


def test_generator_reproduces_fixture(z):
    """the generator run again: with oracle/_ref built through the compiled predictions and with every leaf comparison (MV rate,
    av1_set_ref_frame, av1_drl_ctx, the SSD model, ref_md_sort) and coverage assertion; without it through the numpy predictions"""
    R, L = IP.ref_lib(), G.ref_lib()
    if R is not None and L is not None:
        fresh = G.generate(G.ref_predictor(R), L)
        assert int(fresh["pins"][3]) > 0
    else:
        taps = np.load(os.path.join(ROOT, "tests", "golden", "inter_pred.npz"))["taps"]
        fresh = G.generate(G.np_predictor(taps), None)
    assert set(fresh) == set(z.files)
    for k in z.files:
        if k == "pins":
            assert (fresh[k][:3] == z[k][:3]).all()                          # (the count of compiled sorts depends on the build being there)
            continue
        a, b = np.asarray(fresh[k]), z[k]
        assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), k
