"""GPU: svt_hip_intra_encode_frame (the intra encode pass in coding order: prediction from the reconstructed picture, transform,
quantiser, reconstruction in place) against the fixture (tests/golden/intra_encode.npz: the reference's compiled leaves and the
generator's walk around them), byte for byte, into poisoned outputs: what the call may not write must keep the fill.  The module runs
with two fill bytes (poison.add_second_fill): the planes of the cases without given samples start as the fill, so equal outputs under
both show that no sample the availability rules exclude is read."""
import os
import sys

import numpy as np
import pytest
import torch

import layouts
import poison
from poison import poisoned_outputs  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "intra_encode.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_intra_encode as mi  # noqa: E402

INVALID = -2
OPTIONAL = ("status", "result", "coeff_offset", "sb_qcoeff")
GIVEN = ("inter", "refuse")                                                 # cases whose planes start as given samples


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def tables(dsp):
    return torch.from_numpy(dsp.intra_encode_tables()).to(DEV)


def fill_byte():
    return poison._active.fill_byte


def dev(a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(DEV)


def qrows(c, i):
    return {k: c["qrows"][i][j] for j, k in enumerate(mi.QKEYS)}


def initial_planes(c, name):
    """what the reconstruction planes hold on entry: the given samples, or the fill"""
    return [c[f"init{p}"] if name in GIVEN else np.full(c[f"init{p}"].shape, fill_byte(), np.uint8) for p in range(3)]


def args_of(dsp, tables, c, name, planes=3, optional=OPTIONAL, laid_out=None):
    """the call's dict for case inputs c with fresh poisoned outputs; the planes of all pictures lie in one tensor [npics * rows, stride].
    laid_out = (spec, layouts) of tests/layouts.py: the picture area of every source and reconstruction plane sits at a layout of its
    own instead (views [npics, height, width]); the dict's "placed" lists them for layouts.assert_all_intact"""
    npics, sb_cols, sb_rows, width, height, stride, rows = (int(v) for v in c["dims"])
    nsb = sb_cols * sb_rows
    init = initial_planes(c, name)
    if laid_out is not None:
        return laid_out_args(dsp, tables, c, init, optional, *laid_out)
    recon = []
    for p in range(planes):
        t = poison.tensor((npics * (rows >> (p > 0)), stride >> (p > 0)), torch.uint8, DEV)
        t.copy_(dev(init[p].reshape(t.shape)))
        recon.append(t)
    a = dict(npics=npics, sb_cols=sb_cols, sb_rows=sb_rows, final=dev(c["final"].view(np.uint8).reshape(npics * nsb, mi.MAX_FINAL, 12)),
             final_count=dev(c["count"].reshape(-1)), blk=dev(c["blk"].view(np.uint8).reshape(-1, 8)),
             src=[dev(c[f"src{p}"].reshape(-1, stride >> (p > 0))) for p in range(planes)], recon=recon,
             width=[width >> (p > 0) for p in range(3)], height=[height >> (p > 0) for p in range(3)],
             src_pic_pitch=[(rows >> (p > 0)) * (stride >> (p > 0)) for p in range(3)], recon_pic_pitch=[(rows >> (p > 0)) * (stride >> (p > 0)) for p in range(3)],
             q_luma=qrows(c, 0), q_chroma=qrows(c, 1), tables=tables,
             scratch=torch.empty((dsp.intra_encode_scratch_bytes(npics, nsb),), dtype=torch.uint8, device=DEV))
    if "status" in optional:
        a["status"] = poison.tensor((npics, nsb, mi.MAX_FINAL), torch.uint8, DEV)
    if "result" in optional:
        a["result"] = poison.tensor((npics, nsb, mi.MAX_FINAL, 8), torch.uint8, DEV)
    if "coeff_offset" in optional:
        a["coeff_offset"] = poison.tensor((npics, nsb, mi.MAX_FINAL, 2), torch.int32, DEV)
    if "sb_qcoeff" in optional:
        a["sb_qcoeff"] = [poison.tensor((npics, nsb, mi.SPAN[p]), torch.int32, DEV) for p in range(planes)]
    return a


def laid_out_args(dsp, tables, c, init, optional, spec, lay):
    npics, sb_cols, sb_rows, width, height, stride, rows = (int(v) for v in c["dims"])
    area = lambda a, p: np.ascontiguousarray(a[:, :height >> (p > 0), :width >> (p > 0)])
    src, p_src = layouts.place_operand(spec, lay, "src", [area(c[f"src{p}"], p) for p in range(3)], npics, fill_byte())
    recon, p_recon = layouts.place_operand(spec, lay, "recon", [area(init[p], p) for p in range(3)], npics, fill_byte())
    a = args_of(dsp, tables, c, "", 3, optional)
    a.update(src=list(src), recon=list(recon), placed=(p_src, p_recon),
             src_stride=[lay[f"src.{q}"].stride for q in "yuv"], stride=[lay[f"recon.{q}"].stride for q in "yuv"],
             src_pic_pitch=[layouts.pitch_of(lay[f"src.{q}"], spec.plane(f"src.{q}")) for q in "yuv"],
             recon_pic_pitch=[layouts.pitch_of(lay[f"recon.{q}"], spec.plane(f"recon.{q}")) for q in "yuv"])
    return a


def run(dsp, a):
    assert dsp.intra_encode_frame(a) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()


def outputs_of(a):
    return list(a["recon"]) + [a[k] for k in ("status", "result", "coeff_offset") if a.get(k) is not None] + list(a.get("sb_qcoeff") or ())


def snapshot(a):
    return [t.clone() for t in outputs_of(a)]


def check(a, c, o, name):
    """every output against the fixture where its mask is set, and what the caller had there everywhere else"""
    fill = fill_byte()
    fill32 = np.frombuffer(bytes([fill] * 4), np.int32)[0]
    live = np.arange(mi.MAX_FINAL)[None, None] < np.minimum(c["count"], mi.MAX_FINAL)[..., None]
    init = initial_planes(c, name)
    for p, t in enumerate(a["recon"]):
        want, mask, was = o[f"recon{p}"], o[f"rmask{p}"], init[p]
        got = t.cpu().numpy()
        if got.ndim == 3:                                                    # laid out: the picture area alone, no sample is written outside it
            assert not mask[:, got.shape[1]:].any() and not mask[:, :, got.shape[2]:].any()
            want, mask, was = (x[:, :got.shape[1], :got.shape[2]] for x in (want, mask, was))
        got = got.reshape(want.shape)
        bad = np.nonzero((got != want) & mask)
        assert not len(bad[0]), (name, p, [b[:8] for b in bad], got[bad][:8], want[bad][:8])
        assert np.array_equal(got[~mask], was[~mask]), (name, p, [b[:8] for b in np.nonzero((got != was) & ~mask)])
    if a.get("status") is not None:
        got = a["status"].cpu().numpy()
        assert np.array_equal(got[live], o["status"][live]), (name, np.nonzero((got != o["status"]) & live), got[live][:32])
        assert (got[~live] == fill).all()
    if a.get("result") is not None:
        got = a["result"].cpu().numpy()
        want = o["result"].view(np.uint8).reshape(got.shape)
        bad = np.nonzero((got != want).any(-1) & o["resmask"])
        assert not len(bad[0]), (name, [b[:8] for b in bad], got[bad][:8], want[bad][:8])
        assert (got[~o["resmask"]] == fill).all(), name
    if a.get("coeff_offset") is not None:
        got = a["coeff_offset"].cpu().numpy().view(np.uint32)
        assert np.array_equal(got[live], o["offset"][live]), (name, np.nonzero((got != o["offset"]) & live[..., None]))
        assert (got[~live].view(np.int32) == fill32).all()
    for p, t in enumerate(a.get("sb_qcoeff") or ()):
        got, want, mask = t.cpu().numpy(), o[f"sbq{p}"], o[f"qmask{p}"]
        bad = np.nonzero((got != want) & mask)
        assert not len(bad[0]), (name, p, [b[:8] for b in bad], got[bad][:8], want[bad][:8])
        assert (got[~mask] == fill32).all(), (name, p)


@pytest.mark.parametrize("k", range(len(mi.CASE_NAMES)), ids=mi.CASE_NAMES)
def test_case_equals_the_fixture(dsp, gold, tables, k):
    c, o = mi.load_case(gold, k)
    a = args_of(dsp, tables, c, mi.CASE_NAMES[k])
    run(dsp, a)
    check(a, c, o, mi.CASE_NAMES[k])


def test_the_two_picture_case_with_every_plane_laid_out_differently_equals_the_fixture(dsp, gold, tables):
    """cover1 (two pictures): src_stride[p] unlike stride[p] for every plane, the chroma strides neither luma's nor luma's >> 1,
    src_pic_pitch[p] unlike recon_pic_pitch[p]: twelve strides and pitches no two of which are equal.  tests/layouts.py asserts that,
    and that a mix-up of them stays inside the planes' own allocations, before anything is uploaded."""
    name = "cover1"
    c, o = mi.load_case(gold, mi.CASE_NAMES.index(name))
    npics, sb_cols, sb_rows, width, height, stride, rows = (int(v) for v in c["dims"])
    spec = layouts.picture_spec("svt_hip_intra_encode_frame", width, height, ("src", "recon"), npics)
    a = args_of(dsp, tables, c, name, laid_out=(spec, layouts.distinct_layouts(spec)))
    assert len(set(a["src_stride"] + a["stride"] + a["src_pic_pitch"] + a["recon_pic_pitch"])) == 12
    run(dsp, a)
    check(a, c, o, name)
    layouts.assert_all_intact(a["placed"][0], fill_byte())
    layouts.assert_all_intact(a["placed"][1], fill_byte(), written=True)


@pytest.mark.parametrize("name", ["cover1", "refuse"])
def test_luma_only_and_without_the_optional_outputs(dsp, gold, tables, name):
    """the same planes, status, results, offsets and stream whatever else the call is asked for; a luma-only call leaves the luma of the
    three-plane call"""
    c, o = mi.load_case(gold, mi.CASE_NAMES.index(name))
    o1 = dict(o, result=o["result"].copy())
    o1["result"]["eob"][..., 1:] = 0                                         # a luma-only call codes no chroma: its eobs stay 0
    for planes, optional in ((1, OPTIONAL), (3, ()), (1, ()), (3, ("status",)), (3, ("coeff_offset", "sb_qcoeff")), (1, ("sb_qcoeff", "result"))):
        a = args_of(dsp, tables, c, name, planes, optional)
        run(dsp, a)
        check(a, c, o if planes == 3 else o1, name)


def test_inter_areas_stay_and_the_offsets_are_recon_finals(dsp, gold, tables):
    """the samples of is_intra 0 entries are left as they are, and the stream offsets equal svt_hip_recon_final_frame's for the same list"""
    import make_golden_recon_final as mr
    from make_golden_md_decide import DEC_DTYPE
    name = "inter"
    c, o = mi.load_case(gold, mi.CASE_NAMES.index(name))
    a = args_of(dsp, tables, c, name)
    run(dsp, a)
    status = a["status"].cpu().numpy()
    live = np.arange(mi.MAX_FINAL)[None, None] < c["count"][..., None]
    assert set(status[live].tolist()) == {mi.OK, mi.R_NOT_INTRA} and (status[live] == mi.R_NOT_INTRA).sum() >= 30
    luma = a["recon"][0].cpu().numpy().reshape(c["init0"].shape)
    for e in c["final"][0][live[0]][status[0][live[0]] == mi.R_NOT_INTRA]:
        x, y, w, h = int(e["x"]), int(e["y"]), mi.BS_W[e["bsize"]], mi.BS_H[e["bsize"]]
        assert np.array_equal(luma[0, y:y + h, x:x + w], c["init0"][0, y:y + h, x:x + w])
    # the same list through svt_hip_recon_final_frame: one source group per block size, records in the order of the groups
    npics, sb_cols, sb_rows, width, height, stride, rows = (int(v) for v in c["dims"])
    nsb = sb_cols * sb_rows
    final = c["final"][0].copy()
    order = np.argsort(final["bsize"][live[0]], kind="stable")
    new_src = np.zeros(len(c["blk"]), np.uint32)
    new_src[final["src"][live[0]][order]] = np.arange(len(order))
    final["src"] = new_src[np.minimum(final["src"], len(c["blk"]) - 1)]
    dec = np.zeros(len(order), DEC_DTYPE)
    groups, at = [], 0
    for b in np.unique(final["bsize"][live[0]]).tolist():
        nb = int((final["bsize"][live[0]] == b).sum())
        cw, ch = max(mi.BS_W[b] // 2, 4), max(mi.BS_H[b] // 2, 4)
        shapes = [(mi.BS_W[b], mi.BS_H[b]), (cw, ch), (cw, ch)]
        groups.append(dict(src_first=at, nblocks=nb, bsize=b, tx_type_uv=0,
                           best_pred=[torch.zeros((nb, h, w), dtype=torch.uint8, device=DEV) for w, h in shapes],
                           best_dqcoeff=[torch.zeros((nb, min(w, 32) * min(h, 32)), dtype=torch.int32, device=DEV) for w, h in shapes]))
        at += nb
    ra = dict(final=dev(final.view(np.uint8).reshape(nsb, mi.MAX_FINAL, 12)), final_count=dev(c["count"][0]), decision=dev(dec.view(np.uint8).reshape(-1, 72)),
              groups=groups, planes=3, recon=[torch.zeros((rows >> (p > 0), stride >> (p > 0)), dtype=torch.uint8, device=DEV) for p in range(3)],
              width=[width, width // 2, width // 2], height=[height, height // 2, height // 2],
              coeff_offset=poison.tensor((nsb, mi.MAX_FINAL, 2), torch.int32, DEV),
              scratch=torch.empty((dsp.recon_final_scratch_bytes(nsb),), dtype=torch.uint8, device=DEV))
    assert dsp.recon_final_frame(ra) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()
    assert torch.equal(ra["coeff_offset"].cpu()[torch.from_numpy(live[0])], a["coeff_offset"][0].cpu()[torch.from_numpy(live[0])])


def test_a_list_that_is_no_tree_ends_in_schedule_status(dsp, gold, tables):
    """twelve entries that alternate a 32x32 and a 16x16 block at one place: ten changes of launch kind where a partition tree has at most
    seven.  The luma schedule (after its 64x64 and 64-sample launches: 0 1 0 1 0 1 0 1 0) reaches the first eight; the rest are reported,
    nothing faults and nothing outside the covered block is written"""
    import make_golden_recon_final as mr
    c, o = mi.load_case(gold, mi.CASE_NAMES.index("sb64"))
    big, small = mr.tile([mr.NONE] * 4)[0][0], mr.tile([mr.S(mr.NONE)] * 4)[0][0]
    c = dict(c, final=c["final"].copy(), count=np.array([[12]], np.uint32), blk=np.repeat(c["blk"][:1], 12))
    c["blk"]["tx_type"], c["blk"]["tx_type_uv"], c["blk"]["uv_mode"] = 0, 0, 0
    for k in range(12):
        c["final"][0, 0, k] = (big if k % 2 == 0 else small, 0, 0, 9 if k % 2 == 0 else 6, 0, k)
    a = args_of(dsp, tables, c, "sb64")
    run(dsp, a)
    assert a["status"].cpu().numpy()[0, 0, :12].tolist() == [mi.OK] * 8 + [mi.R_SCHEDULE] * 4
    fill = fill_byte()
    for p, t in enumerate(a["recon"]):
        got = t.cpu().numpy()
        side = 32 >> (p > 0)
        assert (got[:side, :side] != fill).any() and (got[side:] == fill).all() and (got[:, side:] == fill).all(), p


def test_graph_capture_and_replay(dsp, gold, tables):
    name = "cover0"
    c, o = mi.load_case(gold, mi.CASE_NAMES.index(name))
    a = args_of(dsp, tables, c, name)
    args = dsp.make_intra_encode_args(a)
    first = snapshot(a)
    run(dsp, args)                                                          # warm: nothing is created inside the capture
    check(a, c, o, name)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert dsp.intra_encode_frame(args) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.current_stream().wait_stream(side)
    for t, t0 in zip(outputs_of(a), first):                                 # one replay into fresh outputs
        t.copy_(t0)
    graph.replay()
    torch.cuda.synchronize()
    check(a, c, o, name)


def test_invalid_arguments_are_refused_before_anything_is_enqueued(dsp, gold, tables):
    name = "cover1"
    c, o = mi.load_case(gold, mi.CASE_NAMES.index(name))
    good = args_of(dsp, tables, c, name)
    before = snapshot(good)
    flat = lambda t: t.view(torch.uint8).reshape(-1)
    W, H, stride = int(c["dims"][3]), int(c["dims"][4]), int(c["dims"][5])

    def plane_list(key, p, value):
        return {key: [value if j == p else t for j, t in enumerate(good[key])]}

    def q_with(**change):
        return dict(qrows(c, 0), **{k: np.array(v, np.int16) for k, v in change.items()})

    cases = [("npics 0", dict(npics=0)), ("npics 65536", dict(npics=65536)), ("sb_cols 0", dict(sb_cols=0)), ("sb_rows 0", dict(sb_rows=0)),
             ("nsb above 2^20", dict(sb_cols=1 << 10, sb_rows=(1 << 10) + 1)), ("sb_pitch below nsb", dict(sb_pitch=3)), ("nsrc 0", dict(nsrc=0)),
             ("stride below width", dict(stride=[W - 1, stride // 2, stride // 2])), ("src stride below width", dict(src_stride=[W - 1, stride // 2, stride // 2])),
             ("width 65536", dict(width=[65536, 32768, 32768], stride=[65536, 32768, 32768], src_stride=[65536, 32768, 32768])),
             ("width no multiple of 8", dict(width=[W - 4, W // 2 - 2, W // 2 - 2])), ("height no multiple of 8", dict(height=[H - 4, H // 2 - 2, H // 2 - 2])),
             ("chroma not half the luma", dict(width=[W, W // 2 - 4, W // 2 - 4])),
             ("one chroma recon missing", plane_list("recon", 2, None)), ("one chroma src missing", plane_list("src", 1, None)),
             ("chroma recon without chroma src", dict(src=good["src"][:1])), ("one stream plane missing", plane_list("sb_qcoeff", 1, None)),
             ("src is recon", plane_list("src", 0, good["recon"][0])),
             ("scratch NULL", dict(scratch=None)), ("scratch small", dict(scratch=good["scratch"][:-16])),
             ("scratch misaligned", dict(scratch=good["scratch"][8:], scratch_bytes=good["scratch"].numel())),
             ("q_luma NULL", dict(q_luma=None)), ("q_chroma NULL", dict(q_chroma=None)), ("quant_shift no power of two", dict(q_luma=q_with(quant_shift=[3] * 8)))]
    cases += [(key + " NULL", {key: None}) for key in ("final", "final_count", "blk", "tables")]
    cases += [("recon 0 NULL", plane_list("recon", 0, None)), ("src 0 NULL", plane_list("src", 0, None))]
    cases += [(key + " misaligned", {key: flat(good[key])[2:]}) for key in ("final", "final_count", "coeff_offset")]
    cases += [("blk misaligned", dict(blk=flat(good["blk"])[4:], nsrc=len(c["blk"]) - 1)), ("result misaligned", dict(result=flat(good["result"])[4:])),
              ("tables misaligned", dict(tables=flat(good["tables"])[8:]))]
    cases += [(f"sb_qcoeff {p} misaligned", plane_list("sb_qcoeff", p, flat(good["sb_qcoeff"][p])[8:])) for p in range(3)]
    for name_, change in cases:
        assert dsp.intra_encode_frame(dict(good, **change)) == INVALID, name_
        torch.cuda.synchronize()
        assert all(torch.equal(t, t0) for t, t0 in zip(outputs_of(good), before)), name_
    assert dsp.lib.svt_hip_intra_encode_frame(None, None) == INVALID
    assert dsp.intra_encode_scratch_bytes(0, 4) == 0 and dsp.intra_encode_scratch_bytes(1, 0) == 0 and dsp.intra_encode_scratch_bytes(1, (1 << 20) + 1) == 0
    assert dsp.intra_encode_scratch_bytes(2, 4) == 2 * dsp.intra_encode_scratch_bytes(1, 4) > 0
    assert dsp.intra_encode_launches(2, 2, 3) == 2 + 4 * 15 and dsp.intra_encode_launches(2, 2, 1) == 2 + 4 * 12
    run(dsp, good)
    check(good, c, o, name)


poison.add_second_fill(globals())
