"""GPU: svt_hip_interp_sse_frame / svt_hip_interp_decide_frame / svt_hip_interp_search_frame against tests/golden/interp_search.npz (the
compiled convolve entries, highbd_variance64_c and model_rd_from_sse of the reference behind the generator's glue, see
tests/golden/make_golden_interp_search.py).  Every output is allocated poisoned and fenced (tests/poison.py); every comparison is an
equality."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import layouts
import poison
from poison import poisoned_outputs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_inter_pred as mg  # noqa: E402
import make_golden_interp_search as ms  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = -2
W, H = mg.W, mg.H
_gold = None
_dev = {}


def gold():
    global _gold
    if _gold is None:
        _gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "interp_search.npz")))
    return _gold


def planes(dsp):
    """the padded planes of the picture on the device, uploaded once and never written; views at picture sample (0, 0)"""
    if "planes" not in _dev:
        p = mg.planes_of(8, "random")
        assert mg.planes_crc(p) == int(gold()["planes_crc"][0])
        full = {n: [torch.from_numpy(a).to(dsp.device) for a in p[n]] for n in p}
        _dev["planes"] = {n: [t[mg.PAD[min(k, 1)]:, mg.PAD[min(k, 1)]:] for k, t in enumerate(full[n])] for n in full}
        _dev["strides"] = [t.shape[1] for t in full["src"]]
        _dev["keep"] = full
    return _dev["planes"], _dev["strides"]


def laid_out_planes(dsp, call):
    """the same picture with every plane of the references and of the source at a layout of its own (tests/layouts.py)
    -> (views at sample (0, 0), {"ref": strides, "src": strides}, placed)"""
    spec = layouts.ref_src_spec(call, W, H, mg.PAD)
    return layouts.place_ref_src(spec, layouts.distinct_layouts(spec), mg.planes_of(8, "random"))


def rates(dsp, idx):
    if ("rates", idx) not in _dev:
        _dev[("rates", idx)] = torch.from_numpy(gold()["rates"][idx].copy()).to(dsp.device)
    return _dev[("rates", idx)]


def up(dsp, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dsp.device)


def sse_group(dsp, gi, use_uv, with_sse=True, laid_out=None):
    """laid_out: what laid_out_planes returns, in place of the shared planes"""
    g = gold()
    bw, bh, d, same = (int(v) for v in g["groups"][gi])
    if laid_out is None:
        P, strides = planes(dsp)
        strides = {"ref": strides, "src": strides}
    else:
        P, strides = laid_out[:2]
        assert not same                                   # a source that is list 0's planes would have list 0's strides
    blk = g[f"blk_{gi}"]
    n = len(blk)
    np_ = 3 if use_uv else 1
    out = dict(ref0=P["ref0"][:np_], ref1=P["ref1"][:np_], ref_stride=strides["ref"][:np_], src=P["ref0" if same else "src"][:np_],
               src_stride=strides["ref" if same else "src"][:np_], bwidth=bw, bheight=bh, nblocks=n, blk=up(dsp, blk))
    if with_sse:
        out["sse"] = poison.tensor((n, np_, 9), torch.int32, dsp.device)
    return out


def want_sse(gi, use_uv):
    return gold()[f"sse_{gi}"][:, :3 if use_uv else 1, :]


def sse_np(t):
    return t.cpu().numpy().view(np.uint32)


def decide_group(dsp, bw, bh, sse, ctx, searchable, blk=None, with_out=False):
    n = len(ctx)
    d = dict(bwidth=bw, bheight=bh, nblocks=n, sse=sse, ctx=up(dsp, ctx), searchable=up(dsp, searchable),
             decision=poison.tensor((n, 32), torch.uint8, dsp.device))
    if blk is not None:
        d["blk"] = up(dsp, blk)
        if with_out:
            d["blk_out"] = poison.tensor((n, 16), torch.uint8, dsp.device)
    return d


def dec_np(t):
    return t.cpu().numpy().copy().view(ms.DEC_DTYPE).reshape(-1)


def assert_records(got, want, what):
    want = ms.records(want)
    for f in ms.DEC_DTYPE.names:
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f]).ravel()[:6].tolist(), got[f][:6], want[f][:6])


def ok(dsp, rc):
    assert rc == 0, dsp.lib.svt_hip_last_error().decode()
    torch.cuda.synchronize()


@pytest.mark.parametrize("use_uv", (0, 1))
def test_the_sse_table_of_every_fixture_group_equals_the_fixture(dsp, use_uv):
    """one call per group, so that a failure names the shape and the direction"""
    g = gold()
    for gi in range(len(g["groups"])):
        d = sse_group(dsp, gi, use_uv)
        ok(dsp, dsp.interp_sse_frame([d], W, H, use_uv))
        got, want = sse_np(d["sse"]), want_sse(gi, use_uv)
        bad = np.argwhere((got != want).reshape(len(want), -1).any(axis=1)).ravel()
        assert bad.size == 0, (gi, [int(v) for v in g["groups"][gi]], "blocks", bad[:8].tolist(), got[bad[:1]], want[bad[:1]])


@pytest.mark.parametrize("mode", ms.MODES)
def test_the_decide_call_on_the_fixture_s_real_tables_equals_the_fixture(dsp, mode):
    g = gold()
    for ci, (use_uv, lam, q, rt) in enumerate(ms.REAL_CASES):
        ds = []
        for gi in range(len(g["groups"])):
            bw, bh = int(g["groups"][gi][0]), int(g["groups"][gi][1])
            ds.append(decide_group(dsp, bw, bh, up(dsp, want_sse(gi, use_uv).view(np.int32)), g[f"ctx_{gi}"], g[f"searchable_{gi}"]))
        ok(dsp, dsp.interp_decide_frame(ds, dsp.make_interp_params(lam, q, rates(dsp, rt), use_uv, mode)))
        for gi, d in enumerate(ds):
            assert_records(dec_np(d["decision"]), g[f"dec_{gi}_{ci}_{mode}"], (gi, ci, mode))


@pytest.mark.parametrize("mode", ms.MODES)
def test_the_decide_call_on_the_synthetic_tables_equals_the_fixture(dsp, mode):
    """ties with pair 0, ties of the two vertical candidates, unsearchable blocks, both ends of the model's table, a rate term past 2^32"""
    g = gold()
    for si, (bw, bh) in enumerate(ms.SYN_SHAPES):
        for ci, (lam, q, rt) in enumerate(ms.SYN_CASES):
            for use_uv in (0, 1):
                sse = np.ascontiguousarray(g["syn_sse"][:, :3 if use_uv else 1, :]).view(np.int32)
                d = decide_group(dsp, bw, bh, up(dsp, sse), g["syn_ctx"], g["syn_searchable"])
                ok(dsp, dsp.interp_decide_frame([d], dsp.make_interp_params(lam, q, rates(dsp, rt), use_uv, mode)))
                assert_records(dec_np(d["decision"]), g[f"syn_dec_{si}_{ci}_{use_uv}_{mode}"], (si, ci, use_uv, mode))


@pytest.mark.parametrize("use_uv", (0, 1))
def test_the_one_call_search_equals_the_two_calls_and_the_fixture(dsp, use_uv):
    """table in the scratch, and table in the caller's own buffer; blk_out in place and apart"""
    g = gold()
    ci = 0 if use_uv else 1
    _, lam, q, rt = ms.REAL_CASES[ci]
    prm = dsp.make_interp_params(lam, q, rates(dsp, rt), use_uv, ms.FULL)
    gis = list(range(len(g["groups"])))
    ds = []
    for gi in gis:
        d = sse_group(dsp, gi, use_uv, with_sse=gi % 2 == 0)
        n = d["nblocks"]
        d.update(ctx=up(dsp, g[f"ctx_{gi}"]), searchable=up(dsp, g[f"searchable_{gi}"]), decision=poison.tensor((n, 32), torch.uint8, dsp.device))
        d["blk_out"] = d["blk"] if gi % 3 == 0 else poison.tensor((n, 16), torch.uint8, dsp.device)
        ds.append(d)
    need = dsp.interp_search_scratch_bytes(ds, use_uv)
    assert need == sum((len(g[f"blk_{gi}"]) * (3 if use_uv else 1) * 36 + 15) // 16 * 16 for gi in gis if gi % 2)
    scratch = poison.tensor((need,), torch.uint8, dsp.device)
    rc, _ = dsp.interp_search_frame(ds, W, H, prm, scratch)
    ok(dsp, rc)
    for gi, d in zip(gis, ds):
        bw, bh = int(g["groups"][gi][0]), int(g["groups"][gi][1])
        one = sse_group(dsp, gi, use_uv)
        ok(dsp, dsp.interp_sse_frame([one], W, H, use_uv))
        two = decide_group(dsp, bw, bh, one["sse"], g[f"ctx_{gi}"], g[f"searchable_{gi}"], g[f"blk_{gi}"], with_out=True)
        ok(dsp, dsp.interp_decide_frame([two], prm))
        poison.assert_written(one["sse"])
        if "sse" in d:
            assert torch.equal(d["sse"], one["sse"]), gi
        assert torch.equal(d["decision"], two["decision"]) and torch.equal(d["blk_out"], two["blk_out"]), gi
        if use_uv:
            assert_records(dec_np(d["decision"]), g[f"dec_{gi}_{ci}_{ms.FULL}"], gi)
            if f"winblk_{gi}" in g:
                assert np.array_equal(d["blk_out"].cpu().numpy(), g[f"winblk_{gi}"]), gi


def test_the_search_with_six_different_strides_equals_the_fixture(dsp):
    """ref_stride[3] and src_stride[3] all different and odd, chroma's unrelated to luma's, the nine planes at different places: the SSE
    table and the decision records of a group of BI_PRED blocks, luma and chroma, against the fixture"""
    g = gold()
    ci = 0
    use_uv, lam, q, rt = ms.REAL_CASES[ci]
    assert use_uv
    prm = dsp.make_interp_params(lam, q, rates(dsp, rt), use_uv, ms.FULL)
    gi = next(i for i, r in enumerate(g["groups"]) if int(r[2]) == mg.BI and not int(r[3]))
    lp = laid_out_planes(dsp, "svt_hip_interp_search_frame")
    d = sse_group(dsp, gi, use_uv, laid_out=lp)
    n = d["nblocks"]
    d.update(ctx=up(dsp, g[f"ctx_{gi}"]), searchable=up(dsp, g[f"searchable_{gi}"]), decision=poison.tensor((n, 32), torch.uint8, dsp.device),
             blk_out=poison.tensor((n, 16), torch.uint8, dsp.device))
    rc, _ = dsp.interp_search_frame([d], W, H, prm, poison.tensor((max(16, dsp.interp_search_scratch_bytes([d], use_uv)),), torch.uint8, dsp.device))
    ok(dsp, rc)
    got, want = sse_np(d["sse"]), want_sse(gi, use_uv)
    assert np.array_equal(got, want), (gi, np.argwhere(got != want)[:4].tolist())
    assert_records(dec_np(d["decision"]), g[f"dec_{gi}_{ci}_{ms.FULL}"], gi)
    layouts.assert_all_intact(lp[2], poison._active.fill_byte)


def test_blk_out_fed_to_inter_pred_frame_reproduces_the_fixture_s_winner_prediction(dsp):
    g = gold()
    _, lam, q, rt = ms.REAL_CASES[0]
    gis = [gi for gi in range(len(g["groups"])) if f"winpred_{gi}" in g]
    assert {int(g["groups"][gi][2]) for gi in gis} == {ms.LIST0, ms.LIST1, ms.BI}
    P, strides = planes(dsp)
    for gi in gis:
        bw, bh = int(g["groups"][gi][0]), int(g["groups"][gi][1])
        d = decide_group(dsp, bw, bh, up(dsp, want_sse(gi, 1).view(np.int32)), g[f"ctx_{gi}"], g[f"searchable_{gi}"], g[f"blk_{gi}"], with_out=True)
        ok(dsp, dsp.interp_decide_frame([d], dsp.make_interp_params(lam, q, rates(dsp, rt), 1, ms.FULL)))
        assert np.array_equal(d["blk_out"].cpu().numpy(), g[f"winblk_{gi}"]), gi
        n = d["nblocks"]
        pred = poison.tensor((n, bh, bw), torch.uint8, dsp.device)
        ip = dict(ref0=P["ref0"][0], ref1=P["ref1"][0], ref_stride=strides[0], ss=0, bwidth=bw, bheight=bh, nblocks=n, blk=d["blk_out"], pred=pred)
        ok(dsp, dsp.inter_pred_frame([ip], W, H, 8, 0))
        assert np.array_equal(pred.cpu().numpy(), g[f"winpred_{gi}"]), gi


def test_one_call_with_mixed_groups_and_an_empty_group_equals_the_per_group_calls(dsp):
    """more (group, plane) entries than one launch's table holds"""
    g = gold()
    import __graft_entry__ as ge
    gis = list(range(len(g["groups"])))
    assert 3 * len(gis) > ge.load_package().INTER_PRED_MAX_GROUPS
    ds = [sse_group(dsp, gi, 1) for gi in gis]
    empty = dict(sse_group(dsp, 0, 1), nblocks=0)
    ok(dsp, dsp.interp_sse_frame(ds[:5] + [empty] + ds[5:], W, H, 1))
    for gi, d in zip(gis, ds):
        assert np.array_equal(sse_np(d["sse"]), want_sse(gi, 1)), gi
    assert bool((empty["sse"].view(torch.uint8) == poison.fill_value(torch.uint8)).all())
    # the decide call likewise: all groups and an empty one in one call
    _, lam, q, rt = ms.REAL_CASES[0]
    dd = [decide_group(dsp, int(g["groups"][gi][0]), int(g["groups"][gi][1]), ds[gi]["sse"], g[f"ctx_{gi}"], g[f"searchable_{gi}"]) for gi in gis] * 2
    dd = [dict(d, decision=poison.tensor((d["nblocks"], 32), torch.uint8, dsp.device)) for d in dd]
    assert len(dd) > 32
    e2 = dict(dd[0], nblocks=0, decision=poison.tensor((4, 32), torch.uint8, dsp.device))
    ok(dsp, dsp.interp_decide_frame(dd[:7] + [e2] + dd[7:], dsp.make_interp_params(lam, q, rates(dsp, rt), 1, ms.DUAL_FAST)))
    for k, d in enumerate(dd):
        assert_records(dec_np(d["decision"]), g[f"dec_{k % len(gis)}_0_{ms.DUAL_FAST}"], k)
    assert bool((e2["decision"] == poison.fill_value(torch.uint8)).all())


def test_the_search_captured_in_a_graph_and_replayed_equals_the_direct_call(dsp):
    g = gold()
    _, lam, q, rt = ms.REAL_CASES[0]
    prm = dsp.make_interp_params(lam, q, rates(dsp, rt), 1, ms.DUAL_FAST)
    gis = [0, 4, 8, 17]
    ds = []
    for gi in gis:
        d = sse_group(dsp, gi, 1, with_sse=False)
        d.update(ctx=up(dsp, g[f"ctx_{gi}"]), searchable=up(dsp, g[f"searchable_{gi}"]), decision=poison.tensor((d["nblocks"], 32), torch.uint8, dsp.device))
        ds.append(d)
    arr = dsp.make_interp_search_groups(ds)
    need = dsp.lib.svt_hip_interp_search_scratch_bytes(arr, len(ds), 1)
    scratch = poison.tensor((need,), torch.uint8, dsp.device)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            assert dsp.lib.svt_hip_interp_search_frame(arr, len(ds), W, H, 8, ctypes.byref(prm), ctypes.c_void_p(scratch.data_ptr()), need,
                                                       ctypes.c_void_p(st.cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(st)
    for fill in (0x55, 0xAA):
        scratch.fill_(fill)
        for d in ds:
            d["decision"].fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        for gi, d in zip(gis, ds):
            assert_records(dec_np(d["decision"]), g[f"dec_{gi}_0_{ms.DUAL_FAST}"], (gi, fill))


def test_every_refusal_returns_invalid_and_leaves_the_poisoned_outputs_untouched(dsp):
    g = gold()
    _, lam, q, rt = ms.REAL_CASES[0]

    def off(t, nbytes):
        return t.view(torch.uint8).reshape(-1)[nbytes:]

    def untouched(*ts):
        return all(bool((t.view(torch.uint8) == poison.fill_value(torch.uint8)).all()) for t in ts if t is not None)

    # ---- the table ----
    cases = [("bd 10", None, dict(bd=10)), ("bd 12", None, dict(bd=12)), ("use_uv 2", None, dict(use_uv=2)),
             ("picture width 0", None, dict(w=0)), ("picture height not a multiple of 8", None, dict(h=76)),
             ("bwidth 4", lambda d: d.update(bwidth=4), {}), ("bheight 128", lambda d: d.update(bheight=128), {}),
             ("bwidth 12", lambda d: d.update(bwidth=12), {}), ("block wider than the picture", lambda d: d.update(bwidth=64), dict(w=32)),
             ("d_blk NULL", lambda d: d.update(blk=None, nblocks=4), {}), ("d_blk misaligned", lambda d: d.update(blk=off(d["blk"], 2), nblocks=d["nblocks"] - 1), {}),
             ("d_sse NULL", lambda d: d.update(sse=None), {}), ("d_sse misaligned", lambda d: d.update(sse=off(d["sse"], 2)), {}),
             ("d_ref[0][0] NULL", lambda d: d.update(ref0=[None] + d["ref0"][1:]), {}), ("d_src[0] NULL", lambda d: d.update(src=[None] + d["src"][1:]), {}),
             ("d_ref[0][2] NULL with use_uv", lambda d: d.update(ref0=d["ref0"][:2]), {}), ("d_src[1] NULL with use_uv", lambda d: d.update(src=d["src"][:1]), {}),
             ("nblocks beyond one launch", lambda d: d.update(bwidth=64, bheight=64, nblocks=0x80000000), {})]
    for name, edit, kw in cases:
        good, d = sse_group(dsp, 3, 1), sse_group(dsp, 3, 1)
        sse = d["sse"]
        if edit:
            edit(d)
        rc = dsp.interp_sse_frame([good, d], kw.get("w", W), kw.get("h", H), kw.get("use_uv", 1), kw.get("bd", 8))
        torch.cuda.synchronize()
        assert rc == INVALID and dsp.lib.svt_hip_last_error(), (name, rc)
        assert untouched(good["sse"], sse), name
    d = sse_group(dsp, 3, 0)
    d.update(ref0=d["ref0"][:1], src=d["src"][:1], ref1=None)       # allowed: Y alone without use_uv, no list 1 for LIST_0 blocks
    ok(dsp, dsp.interp_sse_frame([d], W, H, 0))
    assert np.array_equal(sse_np(d["sse"]), want_sse(3, 0))
    assert dsp.lib.svt_hip_interp_sse_frame(None, 1, W, H, 8, 0, None) == INVALID
    assert dsp.lib.svt_hip_interp_sse_frame(None, 0, W, H, 8, 0, None) == 0
    # ---- the walk ----
    bw, bh = int(g["groups"][3][0]), int(g["groups"][3][1])
    sse = up(dsp, want_sse(3, 1).view(np.int32))

    def dgroup():
        return decide_group(dsp, bw, bh, sse, g["ctx_3"], g["searchable_3"], g["blk_3"], with_out=True)

    def prm(**kw):
        p = dsp.make_interp_params(kw.get("lam", lam), kw.get("q", q), rates(dsp, rt), kw.get("use_uv", 1), kw.get("mode", ms.FULL))
        if kw.get("no_rates"):
            p.d_rates = None
        return p

    dcases = [("mode 3", None, dict(mode=3)), ("mode -1", None, dict(mode=-1)), ("use_uv 2", None, dict(use_uv=2)), ("quantiser negative", None, dict(q=-8)),
              ("quantiser above int16", None, dict(q=40000)), ("d_rates NULL", None, dict(no_rates=True)),
              ("bwidth 4", lambda d: d.update(bwidth=4), {}), ("bheight 24", lambda d: d.update(bheight=24), {}),
              ("d_sse NULL", lambda d: d.update(sse=None), {}), ("d_sse misaligned", lambda d: d.update(sse=off(d["sse"], 2)), {}),
              ("d_ctx NULL", lambda d: d.update(ctx=None), {}), ("d_searchable NULL", lambda d: d.update(searchable=None), {}),
              ("d_decision NULL", lambda d: d.update(decision=None, nblocks=d["nblocks"]), {}),
              ("d_decision misaligned", lambda d: d.update(decision=off(d["decision"], 4), nblocks=d["nblocks"] - 1), {}),
              ("d_blk_out without d_blk", lambda d: d.update(blk=None), {}), ("d_blk_out misaligned", lambda d: d.update(blk_out=off(d["blk_out"], 2), nblocks=d["nblocks"] - 1), {})]
    for name, edit, kw in dcases:
        good, d = dgroup(), dgroup()
        outs = (good["decision"], good["blk_out"], d["decision"], d["blk_out"])
        if edit:
            edit(d)
        rc = dsp.interp_decide_frame([good, d], prm(**kw))
        torch.cuda.synchronize()
        assert rc == INVALID and dsp.lib.svt_hip_last_error(), (name, rc)
        assert untouched(*outs), name
    assert dsp.interp_decide_frame([dgroup()], None) == INVALID
    # ---- the one call: a scratch that is missing, misaligned or too small; a bad argument of either stage ----
    def sgroup(with_sse=False):
        d = sse_group(dsp, 3, 1, with_sse=with_sse)
        d.update(ctx=up(dsp, g["ctx_3"]), searchable=up(dsp, g["searchable_3"]), decision=poison.tensor((d["nblocks"], 32), torch.uint8, dsp.device))
        return d

    need = dsp.interp_search_scratch_bytes([sgroup()], 1)
    assert need == (len(g["blk_3"]) * 27 * 4 + 15) // 16 * 16 and dsp.interp_search_scratch_bytes([sgroup(True)], 1) == 0
    big = poison.tensor((need + 32,), torch.uint8, dsp.device)
    for name, scratch, p, edit in (("scratch too small", big[:need - 16], prm(), None), ("scratch misaligned", big[8:], prm(), None),
                                   ("bd 10", big, prm(), "bd"), ("mode 7", big, prm(mode=7), None), ("d_ctx NULL", big, prm(), "ctx")):
        d = sgroup()
        if edit == "ctx":
            d["ctx"] = None
        rc, _ = dsp.interp_search_frame([d], W, H, p, scratch, bd=10 if edit == "bd" else 8)
        torch.cuda.synchronize()
        assert rc == INVALID and dsp.lib.svt_hip_last_error(), (name, rc)
        assert untouched(d["decision"], big), name
    d = sgroup()
    arr = dsp.make_interp_search_groups([d])
    p = prm()
    assert dsp.lib.svt_hip_interp_search_frame(arr, 1, W, H, 8, ctypes.byref(p), None, 0, None) == INVALID          # no scratch at all
    torch.cuda.synchronize()
    assert untouched(d["decision"])
    rc, _ = dsp.interp_search_frame([d], W, H, p, big)                                   # and the unedited call is accepted
    ok(dsp, rc)
    assert_records(dec_np(d["decision"]), g[f"dec_3_0_{ms.FULL}"], "accepted")
