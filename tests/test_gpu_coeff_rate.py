"""GPU: svt_hip_coeff_rate_frame, the coefficient rate of quantised blocks (av1_cost_coeffs_txb without its transform-type term,
av1_cost_skip_txb for eob 0), against the reference's fixture (tests/golden/coeff_rate.npz) and, chained behind svt_hip_full_loop_frame,
against the generator's numpy restatement of the function."""
import os
import sys

import numpy as np
import pytest
import torch

import svtlibs
from svtlibs import TX_H, TX_W, txfm_allowed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "coeff_rate.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_coeff_rate as mg  # noqa: E402

SENT = 0x5a
SENT64 = int.from_bytes(bytes([SENT] * 8), "little")
INVALID = -2


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def sentinel(shape, dt=torch.int64):
    return torch.zeros(shape, dtype=dt, device=DEV).view(torch.uint8).fill_(SENT).view(dt)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def iscans(s, types):
    return dev(np.stack([svtlibs.scan_tables(s, t)[1] for t in types]))


def fixture_group(z, s, type_order=None, blocks=None):
    """(group dict, expected bits int64 [n, T]) of one size of the fixture: blocks (indices into the 24, default all) x types"""
    ftypes = [int(t) for t in z[f"s{s}_types"]]
    types = ftypes if type_order is None else type_order
    perm = [ftypes.index(t) for t in types]
    blocks = np.arange(24) if blocks is None else np.asarray(blocks)
    q = z[f"s{s}_q"][perm][:, blocks].transpose(1, 0, 2)                    # [n, T, NC]
    eob = z[f"s{s}_eob"][perm][:, blocks].T.astype(np.int16)
    want = z[f"s{s}_bits"][perm][:, blocks].T.astype(np.int64)
    n = len(blocks)
    g = dict(tx_size=s, tx_types=types, nblocks=n, qcoeff=dev(q), eob=dev(eob), iscan=iscans(s, types),
             txb_skip_ctx=dev(z[f"s{s}_skip_ctx"][blocks]), dc_sign_ctx=dev(z[f"s{s}_dc_ctx"][blocks]),
             coeff_cost=dev(z[f"s{s}_coeff_cost"]), eob_cost=dev(z[f"s{s}_eob_cost"]), bits=sentinel((n, len(types))))
    return g, want


def run(dsp, groups):
    rc = dsp.coeff_rate_frame(groups)
    torch.cuda.synchronize()
    assert rc == 0, dsp.lib.svt_hip_last_error()


def check(groups, wants):
    for g, w in zip(groups, wants):
        got = g["bits"].cpu().numpy()
        assert not (got == np.int64(SENT64)).any(), (g["tx_size"], "a sentinel survived")
        bad = np.argwhere(got != w)
        assert bad.size == 0, (g["tx_size"], g["tx_types"], bad[:8].tolist(), got[tuple(bad[0])], w[tuple(bad[0])])


def test_golden_fixture_all_sizes_in_one_call(dsp, gold):
    """every fixture case bit for bit: the 19 sizes as groups of one call, then each size again with its types reversed and its blocks
    repeated 11 times in another order (several workgroups of every size, a last workgroup that is not full; 38 groups: two launches)"""
    groups, wants = [], []
    for s in range(19):
        g, w = fixture_group(gold, s)
        groups.append(g); wants.append(w)
    for s in range(19):
        types = [int(t) for t in gold[f"s{s}_types"]][::-1]
        g, w = fixture_group(gold, s, types, (np.arange(24 * 11) * 7) % 24)
        groups.append(g); wants.append(w)
    run(dsp, groups)
    check(groups, wants)


def test_large_groups_run_several_units_per_wave(dsp, gold):
    """the host gives a wave 1 .. 4 wave-units by the group's size (one up to 16 383 units, four from 32 768 up): 8x8 with 17 500
    units (two per wave) and 4x4 with 32 771 units (four per wave, the last workgroup not full), the fixture's blocks repeated"""
    groups, wants = [], []
    for s, n in ((1, 14000), (0, 104867)):
        g, w = fixture_group(gold, s, None, (np.arange(n) * 5) % 24)
        groups.append(g); wants.append(w)
    run(dsp, groups)
    check(groups, wants)


@pytest.mark.parametrize("s,t,b", [(0, 0, 9), (3, 0, 4), (8, 10, 17), (14, 11, 6), (4, 0, 0)])
def test_single_group_of_one_block_and_one_type(dsp, gold, s, t, b):
    g, w = fixture_group(gold, s, [t], [b])
    run(dsp, [g])
    check([g], [w])


def test_empty_groups_and_no_groups(dsp, gold):
    g, w = fixture_group(gold, 7)
    empty = dict(tx_size=2, tx_types=[0, 9], nblocks=0)
    run(dsp, [empty, g, empty])
    check([g], [w])
    run(dsp, [])


def test_type_bits_are_added_only_where_eob_is_positive(dsp, gold):
    rng = np.random.default_rng(5)
    groups, wants = [], []
    for s in (0, 8, 3, 17):
        g, w = fixture_group(gold, s)
        tb = rng.integers(0, 1 << 14, w.shape).astype(np.int32)
        g["type_bits"] = dev(tb)
        eob = g["eob"].cpu().numpy().view(np.uint16)
        assert (eob == 0).any() and (eob > 0).any()
        groups.append(g); wants.append(w + np.where(eob > 0, tb, 0))
    run(dsp, groups)
    check(groups, wants)


def test_chained_behind_the_full_loop_without_a_host_copy(dsp):
    """full_loop_frame writes d_qcoeff / d_eob, this call reads the same tensors; the result is the restatement's of the downloaded
    coefficients"""
    rng = np.random.default_rng(77)
    qrow = {k: np.ascontiguousarray(v[60]) for k, v in svtlibs.quant_tables(8).items()}
    fl, cr = [], []
    for s in (0, 8, 3, 4):
        w, h, n = TX_W[s], TX_H[s], 8
        types = [t for t in range(16) if txfm_allowed(s, t)]
        nc = min(w, 32) * min(h, 32)
        src = rng.integers(0, 256, (n, h, w)).astype(np.uint8)
        pred = np.clip(src.astype(np.int32) + rng.integers(-12, 13, (n, h, w)) * (rng.random((n, 1, 1)) < 0.8), 0, 255).astype(np.uint8)
        isc = iscans(s, types)
        q, eob = sentinel((n, len(types), nc), torch.int32), sentinel((n, len(types)), torch.int16)
        fl.append(dict(src=dev(src), pred=dev(pred), nblocks=n, tx_size=s, tx_types=types, iscan=isc, qcoeff=q, eob=eob,
                       dist=sentinel((n, len(types), 2))))
        cc, ec = mg.tables_of(s)
        cr.append(dict(tx_size=s, tx_types=types, nblocks=n, qcoeff=q, eob=eob, iscan=isc, txb_skip_ctx=dev(rng.integers(0, 13, n).astype(np.uint8)),
                       dc_sign_ctx=dev(rng.integers(0, 3, n).astype(np.uint8)), coeff_cost=dev(cc), eob_cost=dev(ec), bits=sentinel((n, len(types)))))
    assert dsp.full_loop_frame(fl, qrow, 1) == 0, dsp.lib.svt_hip_last_error()
    assert dsp.coeff_rate_frame(cr) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()
    wants, neobs = [], 0
    for g in cr:
        s, q, eob = g["tx_size"], g["qcoeff"].cpu().numpy(), g["eob"].cpu().numpy().view(np.uint16)
        sk, dc = g["txb_skip_ctx"].cpu().numpy(), g["dc_sign_ctx"].cpu().numpy()
        cc, ec = mg.tables_of(s)
        w = np.zeros(eob.shape, np.int64)
        for ti, t in enumerate(g["tx_types"]):
            scan = mg.scan_of(s, t)
            for b in range(g["nblocks"]):
                w[b, ti] = mg.np_cost_coeffs_txb(q[b, ti], int(eob[b, ti]), s, t, int(sk[b]), int(dc[b]), cc, ec, scan)
        neobs += int((eob > 1).sum())
        wants.append(w)
    assert neobs > 100                                                   # the chain carried real coefficients
    check(cr, wants)


def test_graph_capture_and_two_replays(dsp, gold):
    groups, wants = [], []
    for s in (1, 13, 10, 12):
        g, w = fixture_group(gold, s)
        groups.append(g); wants.append(w)
    arr = dsp.make_coeff_rate_groups(groups)
    run(dsp, arr)                                                         # warm: nothing is created inside the capture
    check(groups, wants)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert dsp.coeff_rate_frame(arr) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for g in groups:
            g["bits"].view(torch.uint8).fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        check(groups, wants)


def invalid_cases(g):
    """(name, changes to a valid group) that svt_hip_coeff_rate_frame must reject"""
    off = lambda k, n: g[k].reshape(-1).view(torch.uint8)[n:]              # the same buffer, n bytes in
    return [("tx_size -1", dict(tx_size=-1)), ("tx_size 19", dict(tx_size=19)), ("ntypes 0", dict(ntypes=0)), ("ntypes 17", dict(ntypes=17)),
            ("type not defined for the size", dict(tx_size=3, tx_types=[0, 1])), ("type 16", dict(tx_types=[0, 16])),
            ("duplicate type", dict(tx_types=[0, 0])), ("nblocks * ntypes too large", dict(nblocks=0x7fffffff)),
            ("NULL qcoeff", dict(qcoeff=None)), ("NULL eob", dict(eob=None)), ("NULL iscan", dict(iscan=None)),
            ("NULL txb_skip_ctx", dict(txb_skip_ctx=None)), ("NULL dc_sign_ctx", dict(dc_sign_ctx=None)),
            ("NULL coeff_cost", dict(coeff_cost=None)), ("NULL eob_cost", dict(eob_cost=None)), ("NULL bits", dict(bits=None)),
            ("qcoeff 8-byte aligned", dict(qcoeff=off("qcoeff", 8))), ("iscan 2-byte aligned", dict(iscan=off("iscan", 2))),
            ("bits 4-byte aligned", dict(bits=off("bits", 4))), ("coeff_cost 2-byte aligned", dict(coeff_cost=off("coeff_cost", 2))),
            ("eob 1-byte aligned", dict(eob=off("eob", 1)))]


def test_invalid_arguments_return_before_any_launch(dsp, gold):
    good, w = fixture_group(gold, 1, [0, 10])
    other, _ = fixture_group(gold, 2)
    for name, change in invalid_cases(good):
        bad = dict(good, **change)
        for order in ([other, bad], [bad, other]):                       # the bad group last: nothing before it may have run
            arr = dsp.make_coeff_rate_groups(order)                      # (the wrapper would allocate a missing "bits")
            assert dsp.coeff_rate_frame(arr) == INVALID, name
            torch.cuda.synchronize()
            for g in (good, other):
                assert (g["bits"].cpu().numpy() == np.int64(SENT64)).all(), name
    # an empty group's size and types are validated too
    for change in (dict(tx_size=19), dict(tx_types=[0, 0]), dict(tx_size=4, tx_types=[9])):
        arr = dsp.make_coeff_rate_groups([other, dict(dict(tx_size=1, tx_types=[0], nblocks=0), **change)])
        assert dsp.coeff_rate_frame(arr) == INVALID, change
    assert dsp.lib.svt_hip_coeff_rate_frame(None, 1, None) == INVALID and dsp.lib.svt_hip_coeff_rate_frame(None, -1, None) == INVALID
    torch.cuda.synchronize()
    assert (other["bits"].cpu().numpy() == np.int64(SENT64)).all()
    run(dsp, [good])
    check([good], [w])


def test_out_of_range_contexts_return_and_leave_the_next_call_valid(dsp, gold):
    """contexts and eobs are device data: out-of-range values are clamped on the device (an unspecified cost, no fault)"""
    g, w = fixture_group(gold, 8)
    wild = dict(g, txb_skip_ctx=dev(np.full(24, 255, np.uint8)), dc_sign_ctx=dev(np.arange(24).astype(np.uint8) + 3),
                eob=dev(np.full((24, len(g["tx_types"])), -1, np.int16)), bits=sentinel(w.shape))
    run(dsp, [wild])
    assert not (wild["bits"].cpu().numpy() == np.int64(SENT64)).any()
    run(dsp, [g])
    check([g], [w])
