"""Writes tests/golden/coeff_rate.npz: the coefficient rate of quantised transform blocks, computed by the REFERENCE's own
av1_cost_coeffs_txb (EbRateDistortionCost.c:412-519) in oracle/_ref/libsvtref.so through ctypes, for all 19 transform sizes, the three
scan classes and 24 coefficient patterns each.

What is pinned to what.  av1_cost_coeffs_txb calls two dispatch globals that are NULL after load.  av1_txb_init_levels is pointed at the
reference's exported av1_txb_init_levels_c.  av1_get_nz_map_contexts has ONE implementation in the reference, av1_get_nz_map_contexts_sse2
(ASM_SSE2/encodetxb_sse2.c:470), in a translation unit the oracle build does not contain; it is pointed at a ctypes callback that
holds this file's numpy restatement, np_nz_map_contexts, written from the AV1 specification's get_nz_map_ctx (and read against the
SSE2 code).  So the coefficient-context derivation is pinned to the SPECIFICATION, and everything else (the level map, the eob cost,
base / base_eob / sign / range / Golomb costs, get_br_ctx, the order and the sum) to the REFERENCE's function.  The 2-D context
offsets, Coeff_Base_Ctx_Offset in the specification, are compared with the library's av1_nz_map_ctx_offset before use.

The function reads four fields through candidate_buffer_ptr; the buffers built here are zero-filled bytes with pointers and values at
the offsets below (taken once from an offsetof program compiled against the reference's headers).  The call passes PLANE_TYPE_UV, so
that the function skips its Av1TransformTypeRateEstimation term; the tables therefore sit in the [txs_ctx][1] / [eob_multi_size][1] slots.
Before anything is written the offsets are proven on three blocks whose cost is a sum of table entries written out by hand.

np_cost_coeffs_txb is the numpy restatement of the WHOLE function (tests compare it with the reference on every case, and use it where the
reference is not built).

CPU only; run from the repository root after build():  python tests/golden/make_golden_coeff_rate.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svtlibs  # noqa: E402
from svtlibs import TX_H, TX_W, txfm_allowed  # noqa: E402

OUT = os.path.join(HERE, "coeff_rate.npz")
REF = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")

# ---- offsets (bytes) ----
OFF_BUF_CANDIDATE_PTR = 0             # ModeDecisionCandidateBuffer_s.candidate_ptr
SIZEOF_BUF = 192                      # sizeof(ModeDecisionCandidateBuffer_s)
OFF_CAND_TYPE = 20                    # ModeDecisionCandidate_s.type
OFF_CAND_MD_RATE_PTR = 24             # ModeDecisionCandidate_s.md_rate_estimation_ptr
OFF_CAND_TRANSFORM_TYPE = 148         # ModeDecisionCandidate_s.transform_type[PLANE_TYPES], TxType = uint8_t
SIZEOF_CAND = 416                     # sizeof(ModeDecisionCandidate_s)
OFF_MD_COEFF_FAC_BITS = 799376        # MdRateEstimationContext_s.coeffFacBits[TX_SIZES = 5][PLANE_TYPES = 2]
OFF_MD_EOB_FRAC_BITS = 820536         # MdRateEstimationContext_s.eobFracBits[7][2]
SIZEOF_MD = 834144                    # sizeof(MdRateEstimationContext_s)
COEFF_COST_WORDS = 529                # sizeof(LV_MAP_COEFF_COST) / 4
EOB_COST_WORDS = 22                   # sizeof(LV_MAP_EOB_COST) / 4
PLANE_TYPE_UV, INTRA_MODE = 1, 2
# word offsets of LV_MAP_COEFF_COST's members: txb_skip_cost[13][2], base_eob_cost[4][3], base_cost[42][4], eob_extra_cost[22][2],
# dc_sign_cost[3][2], lps_cost[21][13]
TXB_SKIP, BASE_EOB, BASE, EOB_EXTRA, DC_SIGN, LPS = 0, 26, 38, 206, 250, 256

DCT_DCT, ADST_DCT, IDTX, V_DCT, H_DCT = 0, 1, 9, 10, 11
TYPES = (DCT_DCT, V_DCT, H_DCT, IDTX, ADST_DCT)
NBLOCKS = 24
COST_MAX = 16384                      # table entries in [0, COST_MAX): a 1024-coefficient block stays below 2^31
CLASS_2D, CLASS_HORIZ, CLASS_VERT = 0, 1, 2

# Coeff_Base_Ctx_Offset of the AV1 specification (av1_nz_map_ctx_offset): five patterns, row and column clamped to 4
_SQUARE = [[0, 1, 6, 6, 21], [1, 6, 6, 21, 21], [6, 6, 21, 21, 21], [6, 21, 21, 21, 21], [21, 21, 21, 21, 21]]
_SQUARE4 = [[0, 1, 6, 6, 0], [1, 6, 6, 21, 0], [6, 6, 21, 21, 0], [6, 21, 21, 21, 0], [0, 0, 0, 0, 0]]
_TALL = [[0, 11, 11, 11, 11], [11, 11, 11, 11, 11], [6, 6, 21, 21, 21], [6, 21, 21, 21, 21], [21, 21, 21, 21, 21]]
_TALL4 = [[0, 11, 11, 11, 0], [11, 11, 11, 11, 0], [6, 6, 21, 21, 0], [6, 21, 21, 21, 0], [21, 21, 21, 21, 0]]
_WIDE = [[0, 16, 6, 6, 21], [16, 16, 6, 21, 21], [16, 16, 21, 21, 21], [16, 16, 21, 21, 21], [16, 16, 21, 21, 21]]
_WIDE4 = [[0, 16, 6, 6, 21], [16, 16, 6, 21, 21], [16, 16, 21, 21, 21], [16, 16, 21, 21, 21], [0, 0, 0, 0, 0]]


def _offset_table():
    t = []
    for s in range(19):
        w, h = TX_W[s], TX_H[s]
        t.append((_SQUARE4 if w == 4 else _SQUARE) if w == h else ((_TALL4 if w == 4 else _TALL) if w < h else (_WIDE4 if h == 4 else _WIDE)))
    return np.array(t, np.int8)


NZ_MAP_CTX_OFFSET = _offset_table()


def tx_class(tx_type):
    """tx_type_to_class: V_DCT / V_ADST / V_FLIPADST vertical, H_* horizontal, everything else 2-D"""
    return CLASS_VERT if tx_type in (10, 12, 14) else (CLASS_HORIZ if tx_type in (11, 13, 15) else CLASS_2D)


def packed(s):
    return min(TX_W[s], 32), min(TX_H[s], 32)


def cost_index(s):
    """(txs_ctx, eob_multi_size): (txsize_sqr_map + txsize_sqr_up_map + 1) >> 1 and txsize_log2_minus4"""
    lw, lh = TX_W[s].bit_length() - 3, TX_H[s].bit_length() - 3
    kw, kh = packed(s)
    return (min(lw, lh) + max(lw, lh) + 1) >> 1, (kw * kh).bit_length() - 5


def types_of(s):
    return [t for t in TYPES if txfm_allowed(s, t)]


# ---------------------------------------------------------------------------------------------------------------------------
# numpy restatements
# ---------------------------------------------------------------------------------------------------------------------------
def np_levels(q, s):
    """av1_txb_init_levels: min(|q|, 127) of the packed block in a zero map of (KH + 4) rows of stride KW + 4 (TX_PAD_HOR; no row above
    the block is read)"""
    kw, kh = packed(s)
    lev = np.zeros((kh + 4, kw + 4), np.int64)
    lev[:kh, :kw] = np.minimum(np.abs(np.asarray(q, np.int64).reshape(kh, kw)), 127)
    return lev


def np_nz_map_contexts(lev, scan, eob, s, cls):
    """av1_get_nz_map_contexts as the AV1 specification's get_nz_map_ctx defines it, for every position of the packed block (as the
    SSE2 implementation fills them): int8 [KH * KW].  lev: the padded level map, [>= KH + 4, KW + 4]."""
    kw, kh = packed(s)
    ctx = np.zeros(kh * kw, np.int8)
    if eob == 1:
        return ctx                                   # coeff_contexts[0] = 0, nothing else is read
    m = np.minimum(lev, 3)
    at = lambda dr, dc: m[dr:dr + kh, dc:dc + kw]
    mag = at(0, 1) + at(1, 0)
    rows, cols = np.mgrid[0:kh, 0:kw]
    if cls == CLASS_2D:
        mag = mag + at(1, 1) + at(0, 2) + at(2, 0)
        off = NZ_MAP_CTX_OFFSET[s][np.minimum(rows, 4), np.minimum(cols, 4)].astype(np.int64)
    elif cls == CLASS_HORIZ:
        mag = mag + at(0, 2) + at(0, 3) + at(0, 4)
        off = 26 + 5 * np.minimum(cols, 2)           # SIG_COEF_CONTEXTS_2D + {0, 5, 10} by column
    else:
        mag = mag + at(2, 0) + at(3, 0) + at(4, 0)
        off = 26 + 5 * np.minimum(rows, 2)           # by row
    c = np.minimum((mag + 1) >> 1, 4) + off
    if cls == CLASS_2D:
        c[0, 0] = 0
    ctx[:] = c.reshape(-1)
    last = eob - 1                                   # the last coefficient's context goes by its scan index
    ctx[scan[last]] = 1 if last <= kw * kh // 8 else (2 if last <= kw * kh // 4 else 3)
    return ctx


def np_eob_cost(eob, cls, cc, ec):
    """get_eob_cost (:229-245) with get_eob_pos_token"""
    group_start = [0, 1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 513]
    offset_bits = [0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    pt = max(t for t in range(12) if group_start[t] <= eob)
    cost = int(ec[(11 if cls != CLASS_2D else 0) + pt - 1])
    if offset_bits[pt] > 0:
        bit = ((eob - group_start[pt]) >> (offset_bits[pt] - 1)) & 1
        cost += int(cc[EOB_EXTRA + 2 * pt + bit])
        if offset_bits[pt] > 1:
            cost += 512 * (offset_bits[pt] - 1)
    return cost


def np_cost_coeffs_txb(q, eob, s, tx_type, skip_ctx, dc_ctx, cc, ec, scan):
    """av1_cost_coeffs_txb without its transform-type term; av1_cost_skip_txb for eob 0.  q: the packed block, int32 [KH * KW]"""
    cc = np.asarray(cc, np.int64)
    if eob == 0:
        return int(cc[TXB_SKIP + 2 * skip_ctx + 1])
    kw, kh = packed(s)
    cls = tx_class(tx_type)
    q = np.asarray(q, np.int64)
    lev = np_levels(q, s)
    ctx = np_nz_map_contexts(lev, scan, eob, s, cls).astype(np.int64)
    cost = int(cc[TXB_SKIP + 2 * skip_ctx]) + np_eob_cost(eob, cls, cc, ec)
    for c in range(eob - 1, -1, -1):
        pos = int(scan[c])
        v = int(q[pos])
        level = abs(v)
        if c == eob - 1:
            cost += int(cc[BASE_EOB + 3 * ctx[pos] + min(level, 3) - 1])
        else:
            cost += int(cc[BASE + 4 * ctx[pos] + min(level, 3)])
        if v == 0:
            continue
        cost += int(cc[DC_SIGN + 2 * dc_ctx + (v < 0)]) if c == 0 else 512
        if level > 2:
            row, col = pos // kw, pos % kw
            mag = int(lev[row, col + 1] + lev[row + 1, col])
            if cls == CLASS_2D:
                mag += int(lev[row + 1, col + 1]); near = row < 2 and col < 2
            elif cls == CLASS_HORIZ:
                mag += int(lev[row, col + 2]); near = col == 0
            else:
                mag += int(lev[row + 2, col]); near = row == 0
            mag = min((mag + 1) >> 1, 6)
            br = mag if pos == 0 else (mag + 7 if near else mag + 14)
            cost += int(cc[LPS + 13 * br + min(level - 3, 12)])
            if level >= 15:
                cost += 512 * (2 * (level - 14).bit_length() - 1)
    return cost


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
NZ_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint16, ctypes.c_uint8, ctypes.c_int, ctypes.c_void_p)
_lib = None
_keep = []


def _nz_map_callback(levels, scan, eob, tx_size, cls, out):
    kw, kh = packed(tx_size)
    lev = np.frombuffer(ctypes.string_at(levels, (kh + 4) * (kw + 4)), np.uint8).reshape(kh + 4, kw + 4).astype(np.int64)
    sc = np.frombuffer(ctypes.string_at(scan, 2 * kw * kh), np.int16)
    ctx = np_nz_map_contexts(lev, sc, eob, tx_size, cls)
    ctypes.memmove(out, ctx.ctypes.data, 1 if eob == 1 else ctx.size)


def ref_lib():
    """libsvtref.so with av1_txb_init_levels pointed at the reference's C function and av1_get_nz_map_contexts at the callback above;
    None when it is not built.  The slots are pointed on every call (svtlibs.ref_with_slots: whatever refilled them since the last
    call does not matter)"""
    global _lib
    if not _keep:
        _keep.append(NZ_CB(_nz_map_callback))
    first = _lib is None
    _lib = svtlibs.ref_with_slots({"av1_txb_init_levels": "av1_txb_init_levels_c", "av1_get_nz_map_contexts": _keep[0]}, _lib)
    if first and _lib is not None:
        L = _lib
        L.av1_cost_coeffs_txb.restype = ctypes.c_uint64
        L.av1_cost_coeffs_txb.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint16, ctypes.c_int, ctypes.c_uint8, ctypes.c_int16,
                                          ctypes.c_int16, ctypes.c_uint8]
        L.ref_get_scan.restype = ctypes.POINTER(ctypes.c_int16)
        lib_off = np.frombuffer(ctypes.string_at(ctypes.addressof(ctypes.c_char.in_dll(L, "av1_nz_map_ctx_offset")), 19 * 25), np.int8)
        assert np.array_equal(lib_off.reshape(19, 5, 5), NZ_MAP_CTX_OFFSET), "Coeff_Base_Ctx_Offset differs from the reference's table"
    return _lib


class RefCandidate:
    """the three structs av1_cost_coeffs_txb reads through, as zero-filled byte buffers"""

    def __init__(self):
        self.md = np.zeros(SIZEOF_MD, np.uint8)
        self.cand = np.zeros(SIZEOF_CAND, np.uint8)
        self.buf = np.zeros(SIZEOF_BUF, np.uint8)
        self.cand[OFF_CAND_TYPE] = INTRA_MODE
        self.cand[OFF_CAND_MD_RATE_PTR:OFF_CAND_MD_RATE_PTR + 8].view(np.uint64)[0] = self.md.ctypes.data
        self.buf[OFF_BUF_CANDIDATE_PTR:OFF_BUF_CANDIDATE_PTR + 8].view(np.uint64)[0] = self.cand.ctypes.data

    def cost(self, L, q, eob, s, tx_type, skip_ctx, dc_ctx, cc, ec):
        txs_ctx, eob_multi = cost_index(s)
        self.md[:] = 0
        o = OFF_MD_COEFF_FAC_BITS + (txs_ctx * 2 + PLANE_TYPE_UV) * 4 * COEFF_COST_WORDS
        self.md[o:o + 4 * COEFF_COST_WORDS].view(np.int32)[:] = cc
        o = OFF_MD_EOB_FRAC_BITS + (eob_multi * 2 + PLANE_TYPE_UV) * 4 * EOB_COST_WORDS
        self.md[o:o + 4 * EOB_COST_WORDS].view(np.int32)[:] = ec
        self.cand[OFF_CAND_TRANSFORM_TYPE + PLANE_TYPE_UV] = tx_type
        q = np.ascontiguousarray(q, np.int32)
        return int(L.av1_cost_coeffs_txb(self.buf.ctypes.data, q.ctypes.data, eob, PLANE_TYPE_UV, s, skip_ctx, dc_ctx, 0))


def ref_cost(L, rc, q, eob, s, tx_type, skip_ctx, dc_ctx, cc, ec):
    """Av1TuEstimateCoeffBits' choice: av1_cost_skip_txb (a static inline: one table entry) for eob 0, else the reference's function"""
    if eob == 0:
        return int(cc[TXB_SKIP + 2 * skip_ctx + 1])
    return rc.cost(L, q, eob, s, tx_type, skip_ctx, dc_ctx, cc, ec)


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def tables_of(s):
    rng = np.random.default_rng(8800 + s)
    return rng.integers(0, COST_MAX, COEFF_COST_WORDS).astype(np.int32), rng.integers(0, COST_MAX, EOB_COST_WORDS).astype(np.int32)


def contexts_of(s):
    b = np.arange(NBLOCKS)
    return ((b + s) % 13).astype(np.uint8), ((b + 2 * s) % 3).astype(np.uint8)


def hand_blocks(s, scan):
    """the three hand-computable blocks -> [(q, eob)]"""
    kw, kh = packed(s)
    b1 = np.zeros(kw * kh, np.int32); b1[0] = 1
    b2 = np.zeros(kw * kh, np.int32); b2[0] = -20
    b3 = np.zeros(kw * kh, np.int32); b3[0] = 3; b3[scan[1]] = -1
    return [(b1, 1), (b2, 1), (b3, 2)]


def hand_costs(s, tx_type, skip_ctx, dc_ctx, cc, ec, scan):
    """the three blocks' costs as sums of table entries, written out"""
    kw, kh = packed(s)
    assert tx_class(tx_type) == CLASS_2D and scan[0] == 0 and scan[1] in (1, kw) and kw * kh >= 16
    cc = [int(v) for v in cc]
    skip0, eob1, eob2 = cc[TXB_SKIP + 2 * skip_ctx + 0], int(ec[0]), int(ec[1])          # eob_cost[0][eob_pt - 1]: tokens 1, 2 have no extra bits
    # 1: eob 1, DC = +1: the last coefficient at scan index 0 is context 0, level 1 -> base_eob_cost[0][0]; sign through dc_sign_cost
    c1 = skip0 + eob1 + cc[BASE_EOB + 3 * 0 + 0] + cc[DC_SIGN + 2 * dc_ctx + 0]
    # 2: eob 1, DC = -20: base_eob_cost[0][2]; negative DC; no neighbour, position 0 -> range context 0, base_range 17 -> lps_cost[0][12];
    #    Golomb of 20 - 14 = 6: length 3 -> 5 literal bits
    c2 = skip0 + eob1 + cc[BASE_EOB + 3 * 0 + 2] + cc[DC_SIGN + 2 * dc_ctx + 1] + cc[LPS + 13 * 0 + 12] + 5 * 512
    # 3: eob 2, DC = +3 then -1 at scan index 1 (right of or below the DC): the last coefficient, scan index 1 <= wh / 8, is context 1,
    #    level 1 -> base_eob_cost[1][0], a literal sign bit; the DC is not last: position 0 of a 2-D class is context 0, level 3 ->
    #    base_cost[0][3]; positive DC; its one neighbour has level 1: (1 + 1) >> 1 = 1, position 0 -> range context 1, base_range 0
    c3 = skip0 + eob2 + cc[BASE_EOB + 3 * 1 + 0] + 512 + cc[BASE + 4 * 0 + 3] + cc[DC_SIGN + 2 * dc_ctx + 0] + cc[LPS + 13 * 1 + 0]
    return [c1, c2, c3]


def make_blocks(s, tx_type, scan):
    """-> q int32 [NBLOCKS, KH * KW], eob uint16 [NBLOCKS].  Blocks are drawn in scan order, so that eob is what the quantiser would
    report: one past the last non-zero coefficient."""
    kw, kh = packed(s)
    n = kw * kh
    rng = np.random.default_rng(1000 * s + tx_type + 31)
    sign = lambda k: rng.choice([-1, 1], k)

    def nonzero_last(v):
        if len(v) and v[-1] == 0:
            v[-1] = 1
        return v

    golomb = np.array([15, 16, 17, 18, 21, 22, 29, 30, 45, 46, 77, 78, 141, 142, 269, 270, 525, 526, 1037, 1038, 2061, 2062, 4109, 4110, 8205,
                       8206, 16397, 16398, 32781, 40000])
    pats = []                                                     # values by scan index
    pats.append(np.zeros(0, np.int64))                            # 0: eob 0
    pats.append(np.array([1]))                                    # 1: eob 1, DC = +1
    pats.append(np.array([-20]))                                  # 2: eob 1, DC = -20
    pats.append(np.array([3, -1]))                                # 3: two coefficients
    pats.append(nonzero_last(rng.integers(0, 4, n) * sign(n)))    # 4: eob = full, small levels
    pats.append(nonzero_last((rng.random(n) < 0.1) * rng.integers(1, 30, n) * sign(n)))            # 5: eob = full, sparse
    v = np.zeros(n, np.int64); k = max(n // 8, 3); v[:k] = rng.integers(0, 6, k) * sign(k); v[n - 2] = -2
    pats.append(v[:n - 1])                                        # 6: a dense head and a sparse tail
    pats.append(rng.integers(1, 3, n // 2) * sign(n // 2))        # 7: dense small levels
    pats.append(np.resize(np.arange(3, 15), min(n, 48)) * sign(min(n, 48)))                          # 8: levels 3 .. 14, every lps_cost column
    pats.append(np.resize(golomb, min(n, 60)) * sign(min(n, 60)))  # 9: levels 15 .. 40 000, every Golomb length
    pats.append(-rng.integers(1, 20, n // 2 + 1))                 # 10: all negative
    for e in (n // 8 + 1, n // 8 + 2, n // 4 + 1, n // 4 + 2):    # 11 .. 14: the last coefficient on both sides of the context bands' limits
        pats.append(nonzero_last((rng.random(e) < 0.5) * rng.integers(1, 5, e) * sign(e)))
    while len(pats) < NBLOCKS:                                    # 15 ..: mixtures
        e = int(rng.integers(2, n + 1))
        mags = rng.choice([1, 2, 3, 7, 14, 15, 33, 300, 5000], e, p=[.4, .2, .1, .1, .05, .05, .04, .03, .03])
        pats.append(nonzero_last((rng.random(e) < rng.choice([0.15, 0.5, 0.95])) * mags * sign(e)))
    q = np.zeros((NBLOCKS, n), np.int32)
    eob = np.zeros(NBLOCKS, np.uint16)
    for b, v in enumerate(pats):
        assert len(v) <= n and (len(v) == 0 or v[-1] != 0), b
        q[b, scan[:len(v)]] = v
        eob[b] = len(v)
    return q, eob


def scan_of(s, tx_type):
    return svtlibs.scan_tables(s, tx_type)[0].astype(np.int64)


def gen_size(s, L=None):
    """-> dict of the size's arrays; bits from the reference (L) or, without it, from the restatement"""
    cc, ec = tables_of(s)
    skip, dcs = contexts_of(s)
    types = types_of(s)
    kw, kh = packed(s)
    q = np.zeros((len(types), NBLOCKS, kw * kh), np.int32)
    eob = np.zeros((len(types), NBLOCKS), np.uint16)
    bits = np.zeros((len(types), NBLOCKS), np.uint64)
    rc = RefCandidate() if L is not None else None
    for ti, t in enumerate(types):
        scan = scan_of(s, t)
        if L is not None:
            rs = np.ctypeslib.as_array(L.ref_get_scan(s, t, 0), (kw * kh,))
            assert np.array_equal(rs, scan), (s, t)
        q[ti], eob[ti] = make_blocks(s, t, scan)
        for b in range(NBLOCKS):
            a = (q[ti, b], int(eob[ti, b]), s, t, int(skip[b]), int(dcs[b]), cc, ec)
            bits[ti, b] = ref_cost(L, rc, *a) if L is not None else np_cost_coeffs_txb(*a, scan)
            assert bits[ti, b] < 2 ** 31, (s, t, b)
    return dict(types=np.array(types, np.uint8), q=q, eob=eob, bits=bits, coeff_cost=cc, eob_cost=ec, skip_ctx=skip, dc_ctx=dcs)


def prove_offsets(L):
    """the three hand-computed blocks through the reference's function, on a 4x4, an 8x8 and a 16x32: refuses (raises) on any difference"""
    rc = RefCandidate()
    for s in (0, 1, 9):
        cc, ec = tables_of(s)
        scan = scan_of(s, DCT_DCT)
        for sk, dc in ((0, 0), (7, 2), (12, 1)):
            want = hand_costs(s, DCT_DCT, sk, dc, cc, ec, scan)
            for (qb, e), w in zip(hand_blocks(s, scan), want):
                got = rc.cost(L, qb, e, s, DCT_DCT, sk, dc, cc, ec)
                if got != w:
                    raise SystemExit(f"offset proof failed: size {s} contexts {sk}/{dc} eob {e}: reference {got}, by hand {w}")


def main():
    L = ref_lib()
    if L is None:
        raise SystemExit("oracle/_ref/libsvtref.so is not built")
    prove_offsets(L)
    out = {}
    for s in range(19):
        for k, v in gen_size(s, L).items():
            out[f"s{s}_{k}"] = v
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
