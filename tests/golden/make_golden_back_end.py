"""Writes tests/golden/back_end.npz: the back half of the encoder on ONE real picture, stage by stage, each stage fed by the reference's
output of the stage before - what the chain svt_hip_partition_decide_frame -> svt_hip_recon_final_frame -> svt_hip_intra_encode_frame ->
svt_hip_dlf_mi_frame -> svt_hip_dlf_search_frame / svt_hip_dlf_pick_level -> svt_hip_dlf_apply_frame -> svt_hip_cdef_search_frame /
_apply_frame must reproduce when every call reads what the call before it wrote.

Nothing here derives a reference rule: every stage is a sibling generator's route to the reference.
  picture    the 352 x 224 window of real_picture.npz (6 x 4 superblocks, the right column and the bottom row partial) and its list-0
             reference picture (make_golden_real_picture.input_pictures: the window displaced by DISP[0], coded by the reference).  No
             source sample is stored.
  partition  make_golden_partition.ref_partition (Initialize_cu_data_structure, d1_non_square_block_decision,
             d2_inter_depth_block_decision compiled, the generator's loop and encode-pass walk), asserted equal to np_partition, on the
             leaf lists and integer costs of tests/back_end_cases.py.
  recon      inter entries are copied predictions (svt_hip_recon_final_frame with eob 0); then make_golden_intra_encode.model on a
             case built from the final list and back_end_cases.src_tables, with both quantiser rows of one qindex of
             svtlibs.quant_tables(8).  The model is run twice with different samples under the intra blocks: equal outputs show that
             the reference reads no sample of a block that is not yet coded.
  mode info  back_end_cases.info_table / mi_grid (skip by update_av1_mi_map's rule).
  deblock    dlf_cases.ref_pick (av1_pick_filter_level, LPF_PICK_FROM_FULL_IMAGE) from two start rows, ref_table at the sharpness the
             pick stores, ref_frame at the picked levels and once more with ref / mode deltas (back_end_cases.delta_of).
  CDEF       make_golden_cdef.ref_search / ref_apply on the deblocked planes with the skip map of the same grid, the argmin of
             make_golden_real_picture.argmin_strengths.
The coverage conditions of back_end_cases.conditions are asserted; the qindex walks make_golden_real_picture.QINDEX_ORDER until all
hold, and the file is not written otherwise.  Pictures are stored as differences to the stage before, masks as bits.

CPU only; run from the repository root after build():  python tests/golden/make_golden_back_end.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import svtlibs                              # noqa: E402
import back_end_cases as bc                 # noqa: E402
import dlf_cases as dc                      # noqa: E402
import make_golden_cdef as mg_cdef          # noqa: E402
import make_golden_intra_encode as mi       # noqa: E402
import make_golden_partition as mg          # noqa: E402
import make_golden_real_picture as mg_real  # noqa: E402

OUT = bc.FIXTURE
assert (mg_real.W, mg_real.H, mg_real.SIZE_CAP) == (bc.W, bc.H, bc.SIZE_CAP)


def libraries_built():
    return mg.ref_lib() is not None and dc.ref_dlf() is not None


def quantiser_rows(qindex):
    qt = svtlibs.quant_tables(8)
    return np.stack([np.stack([qt[k][qindex] for k in mi.QKEYS])] * 2)


def intra_case(final, count, tabs, pics, init, qindex):
    """make_golden_intra_encode's case dict (the shape of its `inter` case: init* holds the inter samples)"""
    c = dict(dims=np.array([1, bc.SB_COLS, bc.SB_ROWS, bc.W, bc.H, bc.STRIDE, bc.ROWS], np.uint32), final=final[None], count=count[None],
             blk=tabs["blk"], qrows=quantiser_rows(qindex))
    for p, s in enumerate(bc.in_planes(pics["src"])):
        c[f"src{p}"], c[f"init{p}"] = s[None], init[p][None]
    return c


def stage_partition(geom, pics):
    L = mg.ref_lib()
    assert np.array_equal(mg.ref_geometry(L), geom), "the geometry recorded in partition.npz is not the reference's"
    case, groups = bc.partition_case(pics, geom)
    sq, count, final = mg.ref_partition(L, case, geom)
    n_sq, n_count, n_final = mg.np_partition(case, geom)
    assert np.array_equal(sq, n_sq) and np.array_equal(count, n_count) and np.array_equal(final, n_final)
    assert (final["src"] != mg.NO_SRC).all() and int(count.max()) <= bc.MAX_FINAL
    return dict(part_sq=sq, part_count=count, part_final=final, nsrc=np.array(len(case["leaf"]), np.uint32))


def stage_recon(g, pics, geom, rgeom, qindex):
    final, count, nsrc = bc.padded_final(g["part_final"], g["part_count"]), g["part_count"], int(g["nsrc"])
    tabs = bc.src_tables(final, count, pics, geom, rgeom, nsrc)
    inter, intra = bc.block_masks(final, count, tabs, geom, rgeom)
    assert all(((a | b).all() and not (a & b).any()) for a, b in zip(inter, intra)), "the final list tiles the picture"
    R = mi.Ref()
    outs = []
    for under_intra in (0, 0xFF):                                           # what the planes hold where an intra block will be coded
        init = []
        for p in range(3):
            a = np.full((bc.PH[p], bc.PW[p]), under_intra, np.uint8)
            a[inter[p]] = pics["ref"][p][inter[p]]
            init.append(a)
        outs.append(mi.model(R, intra_case(final, count, tabs, pics, bc.in_planes(init), qindex)))
    o = outs[0]
    live = np.arange(bc.MAX_FINAL)[None] < count[:, None]
    d = {}
    for p in range(3):
        rec, mask = (x[f"recon{p}"][0][:bc.PH[p], :bc.PW[p]] for x in outs), o[f"rmask{p}"][0]
        rec = list(rec)
        assert np.array_equal(rec[0][intra[p]], rec[1][intra[p]]), "the reference read a sample of a block not yet coded"
        assert np.array_equal(mask[:bc.PH[p], :bc.PW[p]], intra[p]) and int(mask.sum()) == int(intra[p].sum())
        assert np.array_equal(rec[0][inter[p]], pics["ref"][p][inter[p]])
        assert np.array_equal(o[f"sbq{p}"], outs[1][f"sbq{p}"]) and np.array_equal(o[f"qmask{p}"], outs[1][f"qmask{p}"])
        d[f"rec{p}"], d[f"imask{p}"], d[f"rmask{p}"] = np.ascontiguousarray(rec[0]), inter[p], intra[p]
        d[f"sbq{p}"], d[f"qmask{p}"] = o[f"sbq{p}"][0], o[f"qmask{p}"][0]
    is_intra = tabs["blk"]["is_intra"][final["src"]].astype(bool) & live
    assert np.array_equal(o["status"][0][live], np.where(is_intra, mi.OK, mi.R_NOT_INTRA)[live]) and np.array_equal(o["resmask"][0], is_intra)
    assert np.array_equal(o["result"], outs[1]["result"])
    d.update(status=o["status"][0], offset=o["offset"][0], result=o["result"][0], resmask=o["resmask"][0])
    d["info"] = bc.info_table(final, count, tabs, d["result"], geom, nsrc)
    d["mi"] = bc.mi_grid(final, count, d["info"], rgeom)
    return d


def stage_deblock(g, pics):
    rec, src, grid = [g[f"rec{p}"] for p in range(3)], [np.ascontiguousarray(s) for s in pics["src"]], g["mi"]
    picks = [dc.ref_pick(bc.dlf_row(start, 0), 0, rec, src, grid, loop_filter_mode=bc.LOOP_FILTER_MODE, tx_mode_only_4x4=bc.ONLY_4X4, is_key_frame=0)
             for start in bc.DLF_STARTS]
    sharp = picks[0][1]
    assert all(s == sharp for _, s in picks)
    levels = np.array([lv for lv, _ in picks], np.int32)
    d = dict(dlf_sharp=np.array(sharp, np.int32), dlf_starts=np.array(bc.DLF_STARTS, np.int32), dlf_levels=levels,
             dlf_table=dc.ref_table(bc.dlf_row((0, 0, 0, 0), sharp), rec, src, grid))
    for name, row in (("dlf", bc.dlf_row(levels[0], sharp)), ("dlfd", bc.dlf_row(levels[0], sharp, bc.delta_of(levels[0])))):
        for p, out in enumerate(dc.ref_frame(row, rec, grid)):
            d[f"{name}{p}"] = out
    return d


def stage_cdef(g, pics, qindex):
    L = mg_cdef.ref_lib()
    rec, src, skip = [g[f"dlf{p}"] for p in range(3)], [np.ascontiguousarray(s) for s in pics["src"]], bc.skip_map(g["mi"])
    mse, count, _, _ = mg_cdef.ref_search(L, rec, src, skip, 8, qindex)
    ys, us = mg_real.argmin_strengths(mse, count)
    d = dict(cdef_mse=mse, cdef_count=count, cdef_ystr=ys, cdef_ustr=us)
    for p, out in enumerate(mg_cdef.ref_apply(L, rec, skip, 8, qindex, ys, us)):
        d[f"cdef{p}"] = out
    return d


def build_fixture(qindex, part=None):
    """every stage at one qindex through the reference -> (dict, {stat: value}, {condition: met}); part: stage_partition's dict of an
    earlier call (it does not depend on the qindex)"""
    geom, rgeom = bc.geometry()
    pics = bc.pictures()
    g = dict(origin=pics["origin"], qindex=np.array(qindex, np.int32))
    for p in range(3):
        g[f"src{p}"], g[f"ref{p}"] = pics["src"][p], pics["ref"][p]
    g.update(part if part is not None else stage_partition(geom, pics))
    g.update(stage_recon(g, pics, geom, rgeom, qindex))
    g.update(stage_deblock(g, pics))
    g.update(stage_cdef(g, pics, qindex))
    vals = bc.measure(g, geom, rgeom)
    g["stat_names"], g["stats"] = np.array(bc.STAT_NAMES), np.array([vals[n] for n in bc.STAT_NAMES], np.float64)
    return g, vals, bc.conditions(vals)


def main():
    if mg.ref_lib() is None:
        raise SystemExit("oracle/_ref/libsvtref.so is not built")
    if dc.ref_dlf() is None:
        import make_golden_dlf
        make_golden_dlf.build_ref_lib()
        del dc._lib[:]
    g, part = None, None
    for qindex in mg_real.QINDEX_ORDER:
        cand, vals, met = build_fixture(qindex, part)
        part = {k: cand[k] for k in ("part_sq", "part_count", "part_final", "nsrc")}
        missed = [k for k, ok in met.items() if not ok]
        print(f"qindex {qindex}: " + ("every condition holds" if not missed else "misses " + "; ".join(missed)))
        if not missed:
            g = cand
            break
    assert g is not None, "no qindex of QINDEX_ORDER meets the conditions on this window"
    np.savez_compressed(OUT, **bc.pack(g))
    size = os.path.getsize(OUT)
    back = bc.load(OUT)
    assert sorted(back) == sorted(g), sorted(set(back) ^ set(g))
    assert all(np.array_equal(back[k], g[k]) and back[k].dtype == g[k].dtype for k in g), [k for k in g if not np.array_equal(back[k], g[k]) or back[k].dtype != g[k].dtype]
    for n, v in zip(bc.STAT_NAMES, g["stats"]):
        print(f"  {n} = {v:.4g}")
    print(f"wrote {OUT}: {size} bytes, origin {tuple(int(v) for v in g['origin'])}, qindex {int(g['qindex'])}, levels {g['dlf_levels'].tolist()}")
    assert size < bc.SIZE_CAP, size


if __name__ == "__main__":
    main()
