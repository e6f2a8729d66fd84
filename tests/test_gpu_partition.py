"""GPU: svt_hip_partition_decide_frame (the d1 / d2 partition decision per superblock and the final block list) against the fixture
(tests/golden/partition.npz: the reference's d1_non_square_block_decision and d2_inter_depth_block_decision run whole, the generator's
loop around them and its encode pass walk), byte for byte, into poisoned outputs."""
import os
import sys

import numpy as np
import pytest
import torch

import poison
from poison import poisoned_outputs  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "partition.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_partition as mg  # noqa: E402
import make_golden_md_decide as mgd  # noqa: E402

INVALID = -2
FILL = 0x5A
OUT_KEYS = ("sq", "final_count", "final", "final_decision")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def dev(a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)      # torch has the signed types
    return torch.from_numpy(a.view(view) if view else a).to(DEV)


def records_of(cost):
    """svt_hip_md_decision records that carry the costs, every other member a function of the index"""
    d = np.zeros(len(cost), mgd.DEC_DTYPE)
    i = np.arange(len(cost))
    d["cost"], d["cost_luma"], d["full_lambda_rate"], d["full_distortion"] = cost, i * 3 + 1, i * 7 + 2, i * 11 + 3
    d["eob"][:, 0], d["slot"], d["cand"], d["tx_type"] = i % 1000, i % 40, i % 64, i % 16
    return d


def args_of(c, source="cost", final_decision=False, sbs=None):
    """the call's dict for case inputs c, with fresh poisoned outputs; sbs selects superblocks (the leaf and cost arrays stay whole)"""
    sb = c["sb"] if sbs is None else c["sb"][list(sbs)]
    nsb = len(sb)
    a = dict(sb=dev(sb.view(np.uint8).reshape(nsb, 12)), leaf=dev(c["leaf"].view(np.uint8).reshape(-1, 12)), partition_bits=dev(c["bits"]),
             pic_width=int(c["pic_width"]), pic_height=int(c["pic_height"]), slice_is_intra=int(c["slice_is_intra"]),
             sq=poison.tensor((nsb, mg.NSQ, 16), torch.uint8, DEV), final_count=poison.tensor((nsb,), torch.int32, DEV),
             final=poison.tensor((nsb, mg.MAX_FINAL, 12), torch.uint8, DEV))
    a["lambda"] = int(c["lam"])
    if source == "cost":
        a["cost"] = dev(c["cost"])
    else:
        a["decision"] = dev(records_of(c["cost"]).view(np.uint8).reshape(-1, 72))
    if final_decision:
        a["final_decision"] = poison.tensor((nsb, mg.MAX_FINAL, 72), torch.uint8, DEV)
    return a


def run(dsp, a):
    assert dsp.partition_decide_frame(a) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()


def check(a, sq, count, final, records=None):
    """the outputs against the expected squares [nsb, 341], counts [nsb] and final blocks (concatenated), byte for byte; past each count the
    poison must have survived"""
    got_sq = a["sq"].cpu().numpy().view(mg.SQ_DTYPE).reshape(-1, mg.NSQ)
    bad = np.nonzero(got_sq != sq)
    assert not len(bad[0]), (bad[0][:8], bad[1][:8], got_sq[bad][:4], sq[bad][:4])
    got_count = a["final_count"].cpu().numpy().view(np.uint32)
    assert np.array_equal(got_count, count), (got_count, count)
    got_final = a["final"].cpu().numpy()
    got_dec = a["final_decision"].cpu().numpy() if a.get("final_decision") is not None else None
    at = 0
    for i, n in enumerate(count.tolist()):
        want = final[at:at + n]
        rows = got_final[i, :n].copy().view(mg.FINAL_DTYPE).reshape(-1)
        assert np.array_equal(rows, want), (i, rows[:4], want[:4])
        assert (got_final[i, n:] == FILL).all(), i
        if got_dec is not None:
            src = want["src"].astype(np.int64)
            want_dec = np.where((src == mg.NO_SRC)[:, None], np.uint8(0), records.view(np.uint8).reshape(-1, 72)[np.minimum(src, len(records) - 1)])
            assert np.array_equal(got_dec[i, :n], want_dec), i
            assert (got_dec[i, n:] == FILL).all(), i
        at += n


def untouched(a):
    return all(bool((a[k].view(torch.uint8) == FILL).all()) for k in OUT_KEYS if a.get(k) is not None)


@pytest.mark.parametrize("source", ["cost", "decision"])
@pytest.mark.parametrize("k", range(mg.NCASES), ids=mg.CASE_NAMES)
def test_case_equals_the_fixture(dsp, gold, k, source):
    c, sq, count, final = mg.load_case(gold, k)
    a = args_of(c, source, final_decision=source == "decision")
    run(dsp, a)
    check(a, sq, count, final, records_of(c["cost"]))


def test_without_the_gathered_records(dsp, gold):
    """d_decision as the source, no d_final_decision"""
    c, sq, count, final = mg.load_case(gold, mg.CASE_NAMES.index("edges"))
    a = args_of(c, "decision")
    run(dsp, a)
    check(a, sq, count, final)


def test_all_superblocks_in_one_call_and_one_alone(dsp, gold):
    """46 superblocks: eleven workgroups of four waves and a partial one; then nsb 1, a workgroup with one live wave"""
    c, sq, count, final = mg.load_case(gold, mg.COMBINED)
    assert len(c["sb"]) % 4 == 2
    a = args_of(c, "decision", final_decision=True)
    run(dsp, a)
    check(a, sq, count, final, records_of(c["cost"]))
    ends = np.cumsum(count)
    for i in (6, len(count) - 1):                                           # the 256-block superblock; the last one
        one = args_of(c, "cost", sbs=[i])
        run(dsp, one)
        check(one, sq[i:i + 1], count[i:i + 1], final[ends[i] - count[i]:ends[i]])


def test_src_is_honoured(dsp, gold):
    """the same lists with another permutation of src (and the costs moved with it) give the same squares, and final blocks that name
    the new src"""
    c, sq, count, final = mg.load_case(gold, mg.CASE_NAMES.index("irregular"))
    rng = np.random.default_rng(77)
    perm = rng.permutation(len(c["cost"])).astype(np.uint32)               # old src -> new src
    c2 = dict(c, leaf=c["leaf"].copy(), cost=np.zeros_like(c["cost"]))
    c2["leaf"]["src"] = perm[c["leaf"]["src"]]
    c2["cost"][perm] = c["cost"]
    final2 = final.copy()
    final2["src"] = np.where(final["src"] == mg.NO_SRC, mg.NO_SRC, perm[np.minimum(final["src"], len(perm) - 1)])
    assert not np.array_equal(final2, final)
    a = args_of(c2, "decision", final_decision=True)
    run(dsp, a)
    check(a, sq, count, final2, records_of(c2["cost"]))


def test_invalid_arguments_are_refused_before_the_launch(dsp, gold):
    c, sq, count, final = mg.load_case(gold, mg.CASE_NAMES.index("squares_h_v"))
    good = args_of(c, "decision", final_decision=True)
    cost = dev(c["cost"])
    flat = lambda t: t.view(torch.uint8).reshape(-1)
    cases = [("nsb 0", dict(nsb=0)), ("nsb above 2^31 / 341", dict(nsb=(1 << 31) // 341 + 1)), ("pic_width 0", dict(pic_width=0)), ("pic_height 0", dict(pic_height=0)),
             ("both sources", dict(cost=cost)), ("no source", dict(decision=None, final_decision=None)), ("records gathered from costs", dict(decision=None, cost=cost)),
             ("leaf NULL", dict(leaf=None, nleaves=len(c["leaf"]))), ("nsrc 0", dict(nsrc=0))]
    cases += [(key + " NULL", {key: None}) for key in ("sb", "partition_bits", "sq", "final_count", "final")]
    cases += [(key + " misaligned", {key: flat(good[key])[4:]}) for key in ("sq", "final_decision", "decision")]
    cases += [(key + " misaligned", {key: flat(good[key])[2:]}) for key in ("sb", "leaf", "partition_bits", "final_count", "final")]
    cases += [("cost misaligned", dict(decision=None, final_decision=None, cost=flat(cost)[4:]))]
    for name, change in cases:
        bad = dict(good, **change)
        for key in ("nsb", "nleaves", "nsrc"):                              # the counts stay those of the valid call
            bad.setdefault(key, {"nsb": len(c["sb"]), "nleaves": len(c["leaf"]), "nsrc": len(c["cost"])}[key])
        assert dsp.partition_decide_frame(bad) == INVALID, name
        torch.cuda.synchronize()
        assert untouched(good), name
    assert dsp.lib.svt_hip_partition_decide_frame(None, None) == INVALID
    run(dsp, good)
    check(good, sq, count, final, records_of(c["cost"]))


def test_graph_capture_and_replay(dsp, gold):
    c, sq, count, final = mg.load_case(gold, mg.CASE_NAMES.index("islice_irregular"))
    a = args_of(c, "decision", final_decision=True)
    args = dsp.make_partition_args(a)
    run(dsp, args)                                                          # warm: nothing is created inside the capture
    check(a, sq, count, final, records_of(c["cost"]))
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert dsp.partition_decide_frame(args) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.current_stream().wait_stream(side)
    for key in OUT_KEYS:
        a[key].view(torch.uint8).fill_(FILL)
    graph.replay()
    torch.cuda.synchronize()
    check(a, sq, count, final, records_of(c["cost"]))


def test_out_of_range_device_data_stays_in_its_own_superblock(dsp, gold):
    """the clamp: an mds_idx of 60 000 and a src of 2^32 - 16 in superblock 2, then a reversed list whose range runs 500 entries past
    nleaves in the last superblock.  Every access stays inside the arrays by construction (indices are clamped before they address
    anything); the call returns normally and every other superblock's outputs are the fixture's"""
    c, sq, count, final = mg.load_case(gold, mg.CASE_NAMES.index("irregular"))
    ends = np.cumsum(count)
    for bad_sb, damage in ((2, "indices"), (len(c["sb"]) - 1, "range")):
        c2 = dict(c, leaf=c["leaf"].copy(), sb=c["sb"].copy())
        lo, n = int(c["sb"]["leaf_first"][bad_sb]), int(c["sb"]["leaf_count"][bad_sb])
        if damage == "indices":
            c2["leaf"]["mds_idx"][lo + n // 2], c2["leaf"]["src"][lo + n // 3] = 60000, 0xFFFFFFF0
        else:
            assert lo + n == len(c["leaf"])
            c2["leaf"][lo:lo + n] = c["leaf"][lo:lo + n][::-1]
            c2["sb"]["leaf_count"][bad_sb] = n + 500
        a = args_of(c2, "decision", final_decision=True)
        run(dsp, a)
        keep = [i for i in range(len(c["sb"])) if i != bad_sb]
        got_sq = a["sq"].cpu().numpy().view(mg.SQ_DTYPE).reshape(-1, mg.NSQ)
        assert np.array_equal(got_sq[keep], sq[keep]), damage
        got_count = a["final_count"].cpu().numpy().view(np.uint32)
        assert np.array_equal(got_count[keep], count[keep]) and int(got_count[bad_sb]) <= mg.MAX_FINAL, damage
        got_final = a["final"].cpu().numpy()
        for i in keep:
            rows = got_final[i, :count[i]].copy().view(mg.FINAL_DTYPE).reshape(-1)
            assert np.array_equal(rows, final[ends[i] - count[i]:ends[i]]) and (got_final[i, count[i]:] == FILL).all(), (damage, i)
        assert (got_final[bad_sb, int(got_count[bad_sb]):] == FILL).all(), damage
