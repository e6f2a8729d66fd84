"""Writes tests/golden/tx_decide.npz: the transform-type decision of ProductFullLoopTxSearch (EbFullLoop.c:927-1124) on synthetic
(dist, eob, bits) tables, and the rows Av1TransformTypeRateEstimation reads for every transform size.

What is pinned to what.  The cost of every (block, type) is the REFERENCE's own av1_tu_calc_cost_luma (EbRateDistortionCost.c:2120-2194)
in oracle/_ref/libsvtref.so through ctypes, and so is the has_coeff bit, read back from the y_has_coeff it ors into the candidate.  The
function reads coeffFacBits through candidate_ptr->md_rate_estimation_ptr; the buffers built here are zero-filled bytes with that
pointer at its offsetof offset (the offsets below were taken once from a program compiled against the reference's headers, as
make_golden_coeff_rate.py's were).  The LOOP GLUE is this file's own, written from EbFullLoop.c: the skip of a non-DCT type whose eob is 0
(:1034), the first strictly smaller cost against a best that starts at UINT64_MAX (:940, :1102), and the record of a block without a
candidate.  The helper svt_hip_tx_type_rate_index is pinned to the reference's Av1TransformTypeRateEstimation (:155-191), called with both
rate tables filled so that an entry's value is its own flat index: the returned value names the row that was read.

np_tx_decide / np_tx_type_rate_index are the numpy restatements tests use where the reference is not built (and compare with it where
it is).

CPU only; run from the repository root after build():  python tests/golden/make_golden_tx_decide.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from svtlibs import TX_H, TX_W, txfm_allowed  # noqa: E402

OUT = os.path.join(HERE, "tx_decide.npz")
REF = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")

# ---- offsets (bytes) ----
OFF_BUF_CANDIDATE_PTR = 0             # ModeDecisionCandidateBuffer_s.candidate_ptr
SIZEOF_BUF = 192                      # sizeof(ModeDecisionCandidateBuffer_s)
OFF_CAND_MD_RATE_PTR = 24             # ModeDecisionCandidate_s.md_rate_estimation_ptr
OFF_CAND_Y_HAS_COEFF = 104            # ModeDecisionCandidate_s.y_has_coeff (uint32_t)
OFF_CAND_PRED_MODE = 108              # ModeDecisionCandidate_s.pred_mode
SIZEOF_CAND = 416                     # sizeof(ModeDecisionCandidate_s)
OFF_MD_INTRA_TX_TYPE = 822248         # MdRateEstimationContext_s.intraTxTypeFacBits[EXT_TX_SETS_INTRA = 3][EXT_TX_SIZES = 4][INTRA_MODES = 13][17]
OFF_MD_INTER_TX_TYPE = 832856         # MdRateEstimationContext_s.interTxTypeFacBits[EXT_TX_SETS_INTER = 4][EXT_TX_SIZES = 4][17]
SIZEOF_MD = 834144                    # sizeof(MdRateEstimationContext_s)
INTRA_DIMS, INTER_DIMS = (3, 4, 13, 17), (4, 4, 17)

U64_MAX = 0xFFFFFFFFFFFFFFFF
DCT_DCT, IDTX = 0, 9
NO_CANDIDATE = 0xFF
LAMBDAS = (1, 29041, 0xFFFFFFFF)      # the smallest, a mid value, the largest full_lambda (uint32 in the reference)
NBLOCKS = 40
# one record per block: svt_hip_tx_decision
DEC_DTYPE = np.dtype([("cost", "<u8"), ("dist", "<u8", (2,)), ("bits", "<u8"), ("eob", "<u2"), ("tx_type", "u1"), ("type_index", "u1"),
                      ("has_coeff", "u1"), ("pad", "u1", (3,))])
assert DEC_DTYPE.itemsize == 40
# av1_ext_tx_used's rows with 5, 7 and 12 types (EbDefinitions.h:1472-1479)
SET5, SET7, SET12 = [0, 1, 2, 3, 9], [0, 1, 2, 3, 9, 10, 11], list(range(12))


# ---------------------------------------------------------------------------------------------------------------------------
# numpy restatements
# ---------------------------------------------------------------------------------------------------------------------------
def np_cost(dist, bits, lam):
    """RDCOST(lambda, bits, dist[DIST_CALC_RESIDUAL]) with LUMA_WEIGHT 1, AV1_COST_PRECISION 0, AV1_PROB_COST_SHIFT 9, RDDIV_BITS 7, in
    uint64 arithmetic that wraps; av1_tu_calc_cost_luma's MIN with the zero-cbf cost, UINT64_MAX, changes nothing.  dist uint64 [.., 2]"""
    dist, bits = np.asarray(dist, np.uint64), np.asarray(bits, np.uint64)
    with np.errstate(over="ignore"):
        return ((bits * np.uint64(lam) + np.uint64(256)) >> np.uint64(9)) + dist[..., 0] * np.uint64(128)


def np_pick(cost, dist, eob, bits, types):
    """the loop glue: cost / eob / bits [n, T], dist [n, T, 2] -> DEC_DTYPE [n]"""
    cost, eob = np.asarray(cost, np.uint64), np.asarray(eob, np.uint16)
    dist, bits = np.asarray(dist, np.uint64), np.asarray(bits, np.uint64)
    types = np.asarray(types, np.uint8)
    n = cost.shape[0]
    c = np.where((eob == 0) & (types[None, :] != DCT_DCT), np.uint64(U64_MAX), cost)      # :1034: the stale cost never passes the strict <
    win = np.argmin(c, axis=1)                                                            # the first of the smallest: the first strict minimum
    rows = np.arange(n)
    none = c[rows, win] == np.uint64(U64_MAX)                                             # nothing passed cost < UINT64_MAX
    d = np.zeros(n, DEC_DTYPE)
    d["cost"] = c[rows, win]
    d["dist"] = np.where(none[:, None], np.uint64(0), dist[rows, win])
    d["bits"] = np.where(none, np.uint64(0), bits[rows, win])
    d["eob"] = np.where(none, 0, eob[rows, win])
    d["tx_type"] = np.where(none, DCT_DCT, types[win])
    d["type_index"] = np.where(none, NO_CANDIDATE, win)
    d["has_coeff"] = d["eob"] != 0
    return d


def np_tx_decide(dist, eob, bits, types, lam):
    """svt_hip_tx_decide_frame for one group -> (DEC_DTYPE [n], cost uint64 [n, T])"""
    cost = np_cost(dist, bits, lam)
    return np_pick(cost, dist, eob, bits, types), cost


def np_gather(dec, coeff):
    """the winner's coefficients, zeros for a winner with eob 0 or no winner.  coeff [n, T, NC] -> [n, NC]"""
    n = coeff.shape[0]
    take = np.where(dec["type_index"] == NO_CANDIDATE, 0, dec["type_index"]).astype(np.int64)
    out = coeff[np.arange(n), take].copy()
    out[dec["eob"] == 0] = 0
    return out


def np_tx_type_rate_index(s, is_inter, reduced):
    """-> (coded, ext_tx_set, square_tx_size): get_ext_tx_set_type / get_ext_tx_set / txsize_sqr_map (EbDefinitions.h:1481-1519)"""
    lw, lh = TX_W[s].bit_length() - 3, TX_H[s].bit_length() - 3
    sqr, up = min(lw, lh), max(lw, lh)
    if up > 3:
        st = 0
    elif up == 3:
        st = 1 if is_inter else 0
    elif reduced:
        st = 1 if is_inter else 2
    elif is_inter:
        st = 4 if sqr == 2 else 5
    else:
        st = 2 if sqr == 2 else 3
    ext = ([0, -1, 2, 1, -1, -1], [0, 3, -1, -1, 2, 1])[1 if is_inter else 0][st]
    return int([1, 2, 5, 7, 12, 16][st] > 1 and ext > 0), ext, sqr


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
_lib = None


def ref_lib():
    global _lib
    if _lib is None and os.path.exists(REF):
        L = ctypes.CDLL(REF)
        L.av1_tu_calc_cost_luma.restype = ctypes.c_uint32
        L.av1_tu_calc_cost_luma.argtypes = [ctypes.c_int16, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        L.Av1TransformTypeRateEstimation.restype = ctypes.c_int32
        L.Av1TransformTypeRateEstimation.argtypes = [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8]
        _lib = L
    return _lib


class RefCandidate:
    """the three structs the two functions read through, as zero-filled byte buffers"""

    def __init__(self):
        self.md = np.zeros(SIZEOF_MD, np.uint8)
        self.cand = np.zeros(SIZEOF_CAND, np.uint8)
        self.buf = np.zeros(SIZEOF_BUF, np.uint8)
        self.cand[OFF_CAND_MD_RATE_PTR:OFF_CAND_MD_RATE_PTR + 8].view(np.uint64)[0] = self.md.ctypes.data
        self.buf[OFF_BUF_CANDIDATE_PTR:OFF_BUF_CANDIDATE_PTR + 8].view(np.uint64)[0] = self.cand.ctypes.data

    def cost(self, L, s, eob, dist2, bits, lam):
        """av1_tu_calc_cost_luma on copies of the caller's values -> (y_full_cost, the y_has_coeff bit of tu_index 0)"""
        d = np.array(dist2, np.uint64)
        b = np.array([bits], np.uint64)
        out = np.zeros(1, np.uint64)
        self.cand[OFF_CAND_Y_HAS_COEFF:OFF_CAND_Y_HAS_COEFF + 4] = 0
        L.av1_tu_calc_cost_luma(0, self.cand.ctypes.data, 0, s, int(eob), d.ctypes.data, b.ctypes.data, out.ctypes.data, int(lam))
        return int(out[0]), int(self.cand[OFF_CAND_Y_HAS_COEFF:OFF_CAND_Y_HAS_COEFF + 4].view(np.uint32)[0])

    def fill_rate_tables(self):
        n_intra, n_inter = int(np.prod(INTRA_DIMS)), int(np.prod(INTER_DIMS))
        self.md[OFF_MD_INTRA_TX_TYPE:OFF_MD_INTRA_TX_TYPE + 4 * n_intra].view(np.int32)[:] = np.arange(n_intra)
        self.md[OFF_MD_INTER_TX_TYPE:OFF_MD_INTER_TX_TYPE + 4 * n_inter].view(np.int32)[:] = np.arange(n_inter)

    def rate_index(self, L, s, is_inter, reduced, intra_dir=7, tx_type=IDTX):
        """Av1TransformTypeRateEstimation on tables whose entries are their own flat index -> (coded, ext_tx_set, square_tx_size)"""
        self.cand[OFF_CAND_PRED_MODE] = intra_dir
        v = int(L.Av1TransformTypeRateEstimation(self.buf.ctypes.data, is_inter, 0, s, tx_type, reduced))
        if v == 0:                                    # flat index 0 is [0][0]..[0]: ext_tx_set 0 is never read
            return 0, None, None
        idx = np.unravel_index(v, INTER_DIMS if is_inter else INTRA_DIMS)
        assert idx[-1] == tx_type and (is_inter or idx[2] == intra_dir), (s, is_inter, reduced, idx)
        return 1, int(idx[0]), int(idx[1])


def ref_costs(L, rc, s, dist, eob, bits, lam):
    """-> cost uint64 [n, T], has_coeff uint8 [n, T] from the reference's function"""
    n, T = eob.shape
    cost, has = np.zeros((n, T), np.uint64), np.zeros((n, T), np.uint8)
    for b in range(n):
        for t in range(T):
            cost[b, t], has[b, t] = rc.cost(L, s, eob[b, t], dist[b, t], bits[b, t], lam)
    return cost, has


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def rounding_pair(lam):
    """-> (a, b, da, db): bits a with dist da (earlier) and bits b with dist db (later) that TIE when bits * lambda is truncated by >> 9
    and that the + 256 rounding orders: the later one is cheaper by 1"""
    for b in range(1, 1200):
        fb, rb = (b * lam) >> 9, (b * lam + 256) >> 9
        if rb != fb:
            continue
        for a in range(1, 1200):
            fa, ra = (a * lam) >> 9, (a * lam + 256) >> 9
            if ra == fa + 1 and (fa - fb) % 128 == 0:
                m = (fa - fb) // 128
                return a, b, 50 + max(-m, 0), 50 + max(m, 0)
    raise AssertionError(lam)


def types_of_case(k):
    """the 19 sizes' lists (case k = size k), then two lists without DCT_DCT"""
    if k >= 19:
        return (1, [IDTX, 1, 10]) if k == 19 else (9, [IDTX])             # 8x8 and 16x32
    allowed = [t for t in range(16) if txfm_allowed(k, t)]
    if len(allowed) < 16:
        return k, allowed                                                  # 1 (a 64 side) or 2 types (a 32 side)
    rng = np.random.default_rng(300 + k)
    pick = (allowed, SET12, SET7, SET5)[k % 4]
    return k, [int(t) for t in rng.permutation(pick)]                      # DCT_DCT anywhere in the list


def make_case(k):
    """-> dict: size, types, lambda, dist [n, T, 2], eob [n, T], bits [n, T] (the synthetic inputs)"""
    s, types = types_of_case(k)
    T, n, lam = len(types), NBLOCKS, LAMBDAS[k % 3]
    rng = np.random.default_rng(7000 + k)
    dist = rng.integers(0, 1 << 40, (n, T, 2)).astype(np.uint64)
    bits = rng.integers(0, 1 << 22, (n, T)).astype(np.uint64)
    eob = (rng.integers(1, 1025, (n, T)) * (rng.random((n, T)) < 0.7)).astype(np.uint16)
    dct = types.index(DCT_DCT) if DCT_DCT in types else -1
    ramp = np.arange(T, dtype=np.uint64)
    # 0: the first type wins, 1: the last type wins (dist decides; all eobs positive)
    for b, d in ((0, ramp), (1, ramp[::-1])):
        dist[b, :, 0] = 1000 + 10 * d; bits[b] = 4096; eob[b] = 5
    # 2: an exact tie of all types: the earliest wins
    dist[2, :, 0] = 777; bits[2] = 999; eob[2] = 3
    # 3: a tie of the two last types below the others
    dist[3, :, 0] = 5000; dist[3, -2:, 0] = 40; bits[3] = 1 << 12; eob[3] = 9
    # 4: a non-DCT type with eob 0 has the lowest computed cost and must lose
    dist[4, :, 0] = 9000 + ramp; bits[4] = 100; eob[4] = 2
    nd = next((i for i, t in enumerate(types) if t != DCT_DCT), None)
    if nd is not None:
        dist[4, nd, 0] = 1; bits[4, nd] = 0; eob[4, nd] = 0
    # 5: DCT_DCT with eob 0 wins on its cost
    dist[5, :, 0] = 9000 + ramp; bits[5] = 100; eob[5] = 2
    if dct >= 0:
        dist[5, dct, 0] = 3; eob[5, dct] = 0
    # 6, 7: all eobs 0: DCT_DCT is the only candidate whatever it costs; without it there is none
    eob[6] = 0; eob[7] = 0
    dist[7, :, 0] = ramp + 1
    if dct >= 0:
        dist[7, dct, 0] = 1 << 39
    # 8: two types that only the + 256 rounding orders (the later one wins; truncation would tie and keep the earlier)
    if T >= 2:
        a, bb, da, db = rounding_pair(lam)
        dist[8, :, 0] = 1 << 41; eob[8] = 7; bits[8] = 0
        dist[8, 0, 0] = da; bits[8, 0] = a
        dist[8, 1, 0] = db; bits[8, 1] = bb
    # 9: the largest rate
    bits[9, T // 2] = (1 << 31) - 1; eob[9, T // 2] = 1024
    # 10: dist * 128 wraps: 2^57 + 2 costs 256 + rate and wins against honest thousands
    dist[10, :, 0] = 3000 + ramp; bits[10] = 0; eob[10] = 1
    dist[10, T - 1, 0] = (1 << 57) + 2
    # 11: every type wraps
    dist[11, :, 0] = (np.uint64(1) << np.uint64(63)) + rng.integers(0, 1 << 20, T).astype(np.uint64); eob[11] = 11
    return dict(size=np.int32(s), types=np.array(types, np.uint8), lam=np.uint64(lam), dist=dist, eob=eob, bits=bits)


NCASES = 21


def gen_case(k, L=None):
    """-> the case's arrays with cost / has / decision from the reference (L) or, without it, from the restatement"""
    c = make_case(k)
    s, types, lam = int(c["size"]), c["types"], int(c["lam"])
    if L is not None:
        cost, has = ref_costs(L, RefCandidate(), s, c["dist"], c["eob"], c["bits"], lam)
    else:
        cost, has = np_cost(c["dist"], c["bits"], lam), (c["eob"] != 0).astype(np.uint8)
    dec = np_pick(cost, c["dist"], c["eob"], c["bits"], types)
    # the winner's has_coeff is the reference's bit for that pair
    won = dec["type_index"] != NO_CANDIDATE
    assert np.array_equal(dec["has_coeff"][won], has[np.arange(len(dec)), dec["type_index"].astype(np.int64) % len(types)][won])
    return dict(c, cost=cost, has=has, decision=dec.view(np.uint8).reshape(-1, DEC_DTYPE.itemsize))


def gen_helper(L=None):
    """-> int32 [19, 2 (is_inter), 2 (reduced set), 3]: coded, ext_tx_set, square_tx_size (-1 where the reference reads no row)"""
    out = np.full((19, 2, 2, 3), -1, np.int32)
    rc = RefCandidate() if L is not None else None
    if rc is not None:
        rc.fill_rate_tables()
    for s in range(19):
        for inter in (0, 1):
            for red in (0, 1):
                if L is not None:
                    coded, ext, sq = rc.rate_index(L, s, inter, red)
                    for dr, ty in ((0, 0), (12, 15)):                      # the row does not depend on the direction or the type
                        assert rc.rate_index(L, s, inter, red, dr, ty) == (coded, ext, sq)
                else:
                    coded, ext, sq = np_tx_type_rate_index(s, inter, red)
                out[s, inter, red] = (coded, ext, sq) if coded else (0, -1, -1)
    return out


def decisions(z, k):
    return z[f"c{k}_decision"].view(DEC_DTYPE).reshape(-1)


def check_conditions(z):
    """the fixture cannot miss the hard paths"""
    sizes, ntypes, lams = set(), set(), set()
    first = last = nondct = tie = zero_loses = dct_zero_wins = all_zero = rounding = wraps = none = False
    maxbits = 0
    for k in range(NCASES):
        s, types, lam = int(z[f"c{k}_size"]), [int(t) for t in z[f"c{k}_types"]], int(z[f"c{k}_lam"])
        dist, eob, bits, cost = z[f"c{k}_dist"], z[f"c{k}_eob"], z[f"c{k}_bits"], z[f"c{k}_cost"]
        dec = decisions(z, k)
        T = len(types)
        sizes.add(s); ntypes.add(T); lams.add(lam)
        maxbits = max(maxbits, int(bits.max()))
        cand = ~((eob == 0) & (np.array(types)[None, :] != DCT_DCT))
        for b in range(len(dec)):
            w = int(dec["type_index"][b])
            if w == NO_CANDIDATE:
                none |= DCT_DCT not in types and not cand[b].any()
                continue
            if T > 1:
                first |= w == 0
                last |= w == T - 1
            nondct |= types[w] != DCT_DCT
            tie |= bool((cost[b, w + 1:][cand[b, w + 1:]] == cost[b, w]).any())
            zero_loses |= bool((cost[b][~cand[b]] < cost[b, w]).any()) and int(cost[b][~cand[b]].min()) == int(cost[b].min())
            dct_zero_wins |= types[w] == DCT_DCT and eob[b, w] == 0 and bool((eob[b] != 0).any())
            all_zero |= not eob[b].any()
            with np.errstate(over="ignore"):
                trunc = ((bits[b] * np.uint64(lam)) >> np.uint64(9)) + dist[b, :, 0] * np.uint64(128)
            tw = int(np.argmin(np.where(cand[b], trunc, np.uint64(U64_MAX))))
            rounding |= tw != w and tw < w and trunc[tw] == trunc[w]
            wraps |= int(dist[b, w, 0]) >= 1 << 57
    assert sizes == set(range(19)), sizes
    assert {1, 2, 16} <= ntypes and ntypes & {5, 7, 12}, ntypes
    assert lams == set(LAMBDAS)
    assert maxbits == (1 << 31) - 1
    assert first and last and nondct and tie and zero_loses and dct_zero_wins and all_zero and rounding and wraps and none, \
        (first, last, nondct, tie, zero_loses, dct_zero_wins, all_zero, rounding, wraps, none)


def main():
    L = ref_lib()
    if L is None:
        raise SystemExit("oracle/_ref/libsvtref.so is not built")
    out = {"helper": gen_helper(L)}
    for k in range(NCASES):
        for key, v in gen_case(k, L).items():
            out[f"c{k}_{key}"] = v
    check_conditions(out)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
