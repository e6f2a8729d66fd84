"""Inputs for the byte pins of the Python mirror's make_* builders (tests/test_mirror_cpu.py, tests/golden/make_golden_mirror.py).

A StubTensor has what a builder reads of a torch tensor (data_ptr, shape, stride, numel, element_size, dim, device) and a fixed address
from a counter, so the records the builders fill are the same bytes on every machine, without a device and without the library.
run_cases(pkg) builds every case and returns {case id: hex of the ctypes array or record}."""
import ctypes


class StubTensor:
    device = "stub"

    def __init__(self, addr, shape, esize=1, strides=None):
        self._addr, self.shape, self._esize = addr, tuple(shape), esize
        if strides is None:
            strides, acc = [], 1
            for s in reversed(self.shape):
                strides.insert(0, acc)
                acc *= s
        self._strides = tuple(strides)

    def data_ptr(self):
        return self._addr

    def stride(self, i=None):
        return self._strides if i is None else self._strides[i]

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def element_size(self):
        return self._esize

    def dim(self):
        return len(self.shape)


class Tensors:
    """a source of stub tensors: every one has its own address and, unless given, its own shape"""

    def __init__(self):
        self.k = 0

    def __call__(self, shape=None, esize=1, strides=None):
        self.k += 1
        return StubTensor(0x7F0000000000 + self.k * 0x10000, shape or (self.k + 1, self.k + 2), esize, strides)


def dicts(T, tensors=(), scalars=(), lists=(), planes=(), required=(), overrides=(), first=3):
    """-> [full, minimal, derived]: every key set (a different value in every scalar, a different tensor for every pointer); the required
    keys alone; everything but the keys that override a default taken from a tensor or a list"""
    full, v = {}, first
    for k in tensors:
        full[k] = T()
    for k in scalars:
        full[k] = v
        v += 1
    for k, n, lo in lists:
        full[k] = [lo + j for j in range(n)]
    for k, n, kind in planes:
        full[k] = [T() for _ in range(n)] if kind == "t" else [v + 10 * j for j in range(n)]
        v += 1
    return [full, {k: full[k] for k in required}, {k: x for k, x in full.items() if k not in overrides}]


def with_planes(g, keys, variant):
    """a copy of g whose plane lists are cut to one entry, emptied, or have a None in the middle"""
    out = dict(g)
    for k in keys:
        if k in g:
            p = list(g[k])
            hole = p if isinstance(p[0], int) else [p[0], None] + p[2:]          # (a stride list has no None)
            out[k] = {"one": p[:1], "none": [], "hole": hole}[variant]
    return out


FULL_LOOP = dict(tensors=("src", "src_xy", "pred", "pred_xy", "iscan", "dist", "eob", "qcoeff", "dqcoeff"),
                 scalars=("src_stride", "pred_stride", "nblocks", "tx_size", "ntypes"), lists=(("tx_types", 5, 1),),
                 required=("nblocks", "tx_size", "tx_types"), overrides=("ntypes",))
TX_SEARCH = dict(FULL_LOOP, tensors=FULL_LOOP["tensors"] + ("txb_skip_ctx", "dc_sign_ctx", "type_bits", "coeff_cost", "eob_cost", "decision",
                                                            "best_qcoeff", "best_dqcoeff"), scalars=FULL_LOOP["scalars"] + ("lambda",))
CFL_SEARCH = dict(tensors=("luma", "xy", "iscan", "coeff_cost", "eob_cost", "dist", "bits", "eob"), scalars=("luma_stride", "nblocks", "tx_size", "tx_type"),
                  planes=(("src", 2, "t"), ("pred", 2, "t"), ("txb_skip_ctx", 2, "t"), ("dc_sign_ctx", 2, "t"), ("src_stride", 2, "s"), ("pred_stride", 2, "s")),
                  required=("nblocks", "tx_size"))
CFL_DECIDE_T = ("alpha_rate", "cfl_mode_bits", "dc_mode_bits", "decision", "alpha_q3_cb", "alpha_q3_cr")
FAST_LOOP = dict(tensors=("src", "src_xy", "top", "left", "blocks", "dist", "pred"), scalars=("src_stride", "neigh_pitch", "nblocks", "tx_size", "ncand"),
                 lists=(("modes", 6, 1), ("deltas", 6, -3)), required=("nblocks", "tx_size", "modes", "deltas"), overrides=("neigh_pitch", "ncand"))
FAST_PICK = dict(tensors=("dist", "dist_cb", "dist_cr", "blk", "rates", "pred", "src_xy", "cand", "sorted", "cost", "rate", "ref_fast_cost", "all_cost",
                          "pred_out", "src_xy_out"),
                 scalars=("tx_size", "bsize", "bsize_uv", "nblocks", "ncand", "use_angle_delta", "nfl", "slice_is_intra", "lambda", "ac_dequant_q3",
                          "intrabc_bits"),
                 lists=(("modes", 7, 2), ("deltas", 7, -3), ("uv_modes", 4, 9), ("uv_deltas", 4, -2)), overrides=("ncand",))
INTERP_SSE = dict(tensors=("blk", "sse"), scalars=("bwidth", "bheight", "nblocks"),
                  planes=(("ref0", 3, "t"), ("ref1", 3, "t"), ("src", 3, "t"), ("ref_stride", 3, "s"), ("src_stride", 3, "s")), overrides=("nblocks",))
INTERP_SEARCH = dict(INTERP_SSE, tensors=INTERP_SSE["tensors"] + ("ctx", "searchable", "decision", "blk_out"))
INTER_FAST_PICK = dict(tensors=("blk", "cand_in", "ctx", "rates", "mv_cost", "dist", "dist_cb", "dist_cr", "intra_cost", "intra_rate", "cand", "sorted",
                                "cost", "rate", "ref_fast_cost", "all_cost", "blk_out", "cand_out", "src_xy_out"),
                       scalars=("bsize", "bsize_uv", "ninter", "nintra", "nfl", "nblocks", "lambda", "ac_dequant_q3", "reference_mode_select",
                                "switchable_motion_mode"), overrides=("nblocks",))
INTER_FAST_SEARCH = dict(INTER_FAST_PICK, tensors=INTER_FAST_PICK["tensors"] + ("intra_pred",),
                         scalars=INTER_FAST_PICK["scalars"] + ("bwidth", "bheight", "use_chroma"),
                         planes=(("ref0", 3, "t"), ("ref1", 3, "t"), ("src", 3, "t"), ("pred_out", 3, "t"), ("ref_stride", 3, "s"), ("src_stride", 3, "s")))
MD_GATHERS = ("pred", "best_pred", "qcoeff", "dqcoeff", "best_qcoeff", "best_dqcoeff")
MD_DECIDE = dict(tensors=("luma", "dist_cb", "dist_cr", "bits_cb", "bits_cr", "eob_cb", "eob_cr", "rate", "cand", "cand_out", "cfl", "blk", "rates",
                          "decision", "full_cost", "inter_blk", "best_inter_blk"),
                 scalars=("bsize", "nblocks", "n", "ninter", "nintra", "lambda", "slice_is_intra", "full_loop_escape"), lists=(("modes", 9, 1),),
                 planes=tuple((k, 3, "t") for k in MD_GATHERS), required=("bsize", "nblocks", "n"))
QROW_A = {"zbin": [11, 12], "round": [13, 14], "quant": [15, 16], "quant_shift": [17, 18], "dequant": [19, 20]}
QROW_B = {k: [x + 20 for x in v] for k, v in QROW_A.items()}
PLANE_KEYS = ("ref0", "ref1", "src", "pred_out", "ref_stride", "src_stride") + MD_GATHERS
MASKED = {"make_recon_final_args": ("groups",), "make_intra_encode_args": ("q_luma", "q_chroma")}      # host addresses: not comparable


def masked_bytes(rec, names):
    """the record's bytes with the named fields zeroed"""
    b = bytearray(bytes(rec))
    for n in names:
        f = getattr(type(rec), n)
        b[f.offset:f.offset + f.size] = bytes(f.size)
    return bytes(b)


def plane_variants(make, spec):
    """the plane-list shapes of one builder: full, minimal and derived dicts, then lists of one, of none and with a hole"""
    gs = dicts(Tensors(), **spec)
    return make(gs + [with_planes(gs[0], PLANE_KEYS, v) for v in ("one", "none", "hole")])


def recon_final_dict(T, groups=True):
    a = dict(final=T(), final_count=T(), decision=T(), recon=[T((40, 64)), T((20, 32)), T((20, 33))], scratch=T((4096,)), status=T(),
             sb_qcoeff=[T(), T(), T()], coeff_offset=T())
    if groups:
        a["groups"] = [dict(src_first=3, nblocks=4, bsize=5, tx_type_uv=6, best_pred=[T(), T(), T()], best_dqcoeff=[T(), T(), T()],
                            best_qcoeff=[T(), T(), T()]),
                       dict(src_first=7, nblocks=8, bsize=9), dict(src_first=1, nblocks=2, bsize=3, best_pred=[T()], best_dqcoeff=[T(), None, T()])]
    return a


def intra_encode_dict(T):
    return dict(sb_cols=3, sb_rows=2, npics=4, sb_pitch=9, blk_pitch=700, final=T(), final_count=T(), blk=T(), src=[T((40, 64)), T((20, 32)), T((20, 33))],
                recon=[T((41, 70)), T((21, 38)), T((22, 39))], tables=T(), scratch=T((999,), 1), status=T(), result=T(), sb_qcoeff=[T(), T(), T()],
                coeff_offset=T(), q_luma=QROW_A, q_chroma=QROW_B)


def md_search_dicts(T, chroma):
    md, luma = dicts(T, **MD_DECIDE)[0], dicts(T, **TX_SEARCH)[0]
    g = {"md": md, "luma": luma}
    if chroma:
        g.update(cb=dicts(T, **FULL_LOOP)[0], cr=dicts(T, **FULL_LOOP)[2], txb_skip_ctx_c=[T(), T()], dc_sign_ctx_c=[T(), T()], coeff_cost_uv=T(),
                 eob_cost_uv=T(), bits_c=[T(), T()])
    return g


def pic_planes(T, stack, esize=1):
    lead = (3,) if stack else ()
    mk = lambda rows, stride: T(lead + (rows, stride), esize, ((rows + 2) * (stride + 8),) * len(lead) + (stride + 8, 1))
    return [mk(48, 64), mk(24, 32), mk(24, 40)]


def cases(dsp):
    """-> [(case id, builder name, thunk -> ctypes array or record)]"""
    c = []

    def add(cid, name, thunk):
        c.append((cid, name, thunk))

    def simple(name, spec, extra=None):
        make = getattr(dsp, name)
        add(name, name, lambda: make(dicts(Tensors(), **spec) + (extra(Tensors()) if extra else [])))
        add(name + "[]", name, lambda: make([]))

    long_types = lambda T: [dict(nblocks=3, tx_size=2, tx_types=list(range(18)), lambda_unused=1), dict(nblocks=3, tx_size=2, tx_types=list(range(16)))]
    simple("make_frame_groups", dict(tensors=("src", "pred", "recon", "xy", "iscan", "qcoeff", "eob", "offsets", "coeff", "dqcoeff"),
                                     scalars=("src_stride", "pred_stride", "recon_stride", "tx_size", "tx_type"),
                                     required=("src_stride", "pred_stride", "recon_stride", "xy", "tx_size", "tx_type")))
    cfl_all = ("luma_recon", "luma_stride", "pred_cb", "cb_stride", "pred_cr", "cr_stride", "xy", "alpha_cb", "alpha_cr", "width", "height")
    simple("make_frame_cfl_groups", dict(tensors=("luma_recon", "pred_cb", "pred_cr", "xy", "alpha_cb", "alpha_cr"),
                                         scalars=("luma_stride", "cb_stride", "cr_stride", "width", "height"), required=cfl_all))
    add("make_frame_levels", "make_frame_levels", lambda: (lambda T: dsp.make_frame_levels([T(), None, T()]))(Tensors()))
    add("make_frame_levels[]", "make_frame_levels", lambda: dsp.make_frame_levels([]))
    simple("make_full_loop_groups", FULL_LOOP, long_types)
    simple("make_coeff_rate_groups", dict(tensors=("qcoeff", "eob", "iscan", "txb_skip_ctx", "dc_sign_ctx", "type_bits", "coeff_cost", "eob_cost", "bits"),
                                          scalars=("tx_size", "ntypes", "nblocks"), lists=(("tx_types", 5, 1),), required=("nblocks", "tx_size", "tx_types"),
                                          overrides=("ntypes",)), long_types)
    simple("make_tx_decide_groups", dict(tensors=("dist", "eob", "bits", "qcoeff", "dqcoeff", "decision", "best_qcoeff", "best_dqcoeff"),
                                         scalars=("tx_size", "ntypes", "nblocks", "lambda"), lists=(("tx_types", 5, 1),),
                                         required=("nblocks", "tx_size", "tx_types"), overrides=("ntypes",)), long_types)
    simple("make_tx_search_groups", TX_SEARCH, long_types)
    pair_holes = lambda T: [dict(nblocks=2, tx_size=1, src=[T(), None], pred=[None, T()], txb_skip_ctx=[T()], src_stride=[5], pred_stride=[])]
    simple("make_cfl_search_groups", CFL_SEARCH, pair_holes)
    simple("make_cfl_decide_groups", dict(tensors=("dist", "bits") + CFL_DECIDE_T, scalars=("nblocks", "lambda"), required=("nblocks",)))
    simple("make_cfl_pick_groups", dict(CFL_SEARCH, tensors=CFL_SEARCH["tensors"] + CFL_DECIDE_T, scalars=CFL_SEARCH["scalars"] + ("lambda",)), pair_holes)
    long_modes = lambda T: [dict(nblocks=2, tx_size=1, modes=list(range(70)), deltas=[-(j % 4) for j in range(70)], uv_modes=list(range(66)))]
    simple("make_fast_loop_groups", FAST_LOOP, long_modes)
    simple("make_fast_pick_groups", FAST_PICK, long_modes)
    simple("make_inter_pred_groups", dict(tensors=("ref0", "ref1", "blk", "pred", "src", "dist"),
                                          scalars=("ref_stride", "ss", "bwidth", "bheight", "nblocks", "pred_stride", "src_stride"), overrides=("nblocks",)))
    simple("make_warp_fit_groups", dict(tensors=("samples", "blk", "model", "nvalid"), scalars=("bsize", "ncand", "nblocks"), overrides=("nblocks",)))
    simple("make_warp_pred_groups", dict(tensors=("ref", "blk", "model", "sel", "pred", "src", "dist"),
                                         scalars=("ref_stride", "ss", "bwidth", "bheight", "nblocks", "ncand", "n", "sel_first", "pred_stride", "src_stride"),
                                         overrides=("nblocks", "n")))
    simple("make_interp_decide_groups", dict(tensors=("sse", "ctx", "searchable", "decision", "blk", "blk_out"), scalars=("bwidth", "bheight", "nblocks"),
                                             overrides=("nblocks",)))
    simple("make_inter_fast_pick_groups", INTER_FAST_PICK)
    for name, spec in (("make_interp_sse_groups", INTERP_SSE), ("make_interp_search_groups", INTERP_SEARCH),
                       ("make_inter_fast_search_groups", INTER_FAST_SEARCH), ("make_md_decide_groups", MD_DECIDE)):
        add(name, name, lambda name=name, spec=spec: plane_variants(getattr(dsp, name), spec))
        add(name + "[]", name, lambda name=name: getattr(dsp, name)([]))

    def numpy_lists(name):
        """host lists given as numpy arrays, as the GPU tests give them"""
        import numpy as np
        u8, i8 = (lambda *v: np.array(v, np.uint8)), (lambda *v: np.array(v, np.int8))
        g = {"make_md_decide_groups": dict(bsize=3, nblocks=4, n=5, modes=u8(1, 2, 3, 9, 12)),
             "make_fast_loop_groups": dict(nblocks=2, tx_size=1, modes=u8(0, 1, 9), deltas=i8(0, -3, 2)),
             "make_fast_pick_groups": dict(modes=u8(0, 1, 9), deltas=i8(0, -3, 2), uv_modes=u8(0, 13), uv_deltas=i8(0, -1)),
             "make_full_loop_groups": dict(nblocks=2, tx_size=1, tx_types=u8(0, 9, 3)),
             "make_interp_sse_groups": dict(ref_stride=np.array([64, 32, 33]), src_stride=np.array([65, 34, 35], np.uint32)),
             "make_inter_fast_search_groups": dict(ref_stride=np.array([64, 32, 33]), src_stride=np.array([65, 34, 35], np.int64))}[name]
        return getattr(dsp, name)([g])

    for name in ("make_md_decide_groups", "make_fast_loop_groups", "make_fast_pick_groups", "make_full_loop_groups", "make_interp_sse_groups",
                 "make_inter_fast_search_groups"):
        add(name + "[numpy]", name, lambda name=name: numpy_lists(name))
    add("make_interp_params", "make_interp_params", lambda: dsp.make_interp_params(3, 4, Tensors()(), 5, 6))
    add("make_interp_params[no rates]", "make_interp_params", lambda: dsp.make_interp_params(7, 8, None, True, 1))

    part = dict(tensors=("sb", "leaf", "decision", "cost", "partition_bits", "sq", "final_count", "final", "final_decision"),
                scalars=("nsb", "nleaves", "nsrc", "lambda", "pic_width", "pic_height", "slice_is_intra"), required=("sb",), overrides=("nsb", "nleaves", "nsrc"))
    for i, label in enumerate(("full", "min", "derived")):
        add(f"make_partition_args[{label}]", "make_partition_args", lambda i=i: dsp.make_partition_args(dicts(Tensors(), **part)[i]))
    add("make_partition_args[cost]", "make_partition_args",
        lambda: dsp.make_partition_args({k: v for k, v in dicts(Tensors(), **part)[2].items() if k != "decision"}))

    def recon_final(variant):
        T = Tensors()
        a = recon_final_dict(T, groups=variant != "no groups")
        if variant == "given":
            a.update(nsb=3, nsrc=4, ngroups=2, planes=1, stride=[100, 50], width=[60], height=[30, 15, 16], scratch_bytes=77)
        elif variant == "min":
            a = dict(final_count=a["final_count"], decision=a["decision"])
        elif variant in ("one", "none", "hole"):
            a = with_planes(a, ("recon", "sb_qcoeff"), variant)
        return dsp.make_recon_final_args(a)

    for v in ("groups", "no groups", "given", "min", "one", "none", "hole"):
        add(f"make_recon_final_args[{v}]", "make_recon_final_args", lambda v=v: recon_final(v))
        add(f"make_recon_final_args[{v}].groups", None, lambda v=v: recon_final(v)._groups)

    def intra_encode(variant):
        a = intra_encode_dict(Tensors())
        if variant == "given":
            a.update(nsrc=55, src_stride=[100, 50, 51], stride=[101], width=[60, 30], height=[30, 15, 16], src_pic_pitch=[7000, 3000, 3001],
                     recon_pic_pitch=[7100, 3100], scratch_bytes=77)
        elif variant == "min":
            a = dict(sb_cols=5, sb_rows=6)
        elif variant == "luma rows":
            del a["q_chroma"]
        elif variant in ("one", "none", "hole"):
            a = with_planes(a, ("src", "recon", "sb_qcoeff"), variant)
        return dsp.make_intra_encode_args(a)

    for v in ("both rows", "luma rows", "given", "min", "one", "none", "hole"):
        add(f"make_intra_encode_args[{v}]", "make_intra_encode_args", lambda v=v: intra_encode(v))

    def md_search():
        T = Tensors()
        with_c, without = md_search_dicts(T, True), md_search_dicts(T, False)
        no_bits = dict(md_search_dicts(T, True))
        del no_bits["bits_c"], no_bits["coeff_cost_uv"]
        return dsp.make_md_search_groups([with_c, without, no_bits])

    def md_search_holes():
        """a None inside the chroma context, bits and gather lists (what the GPU test of bad stage arguments passes)"""
        T = Tensors()
        g = md_search_dicts(T, True)
        g.update(txb_skip_ctx_c=[g["txb_skip_ctx_c"][0], None], dc_sign_ctx_c=[None, g["dc_sign_ctx_c"][1]], bits_c=[None, g["bits_c"][1]])
        g["md"] = dict(g["md"], decision=None, rates=None, best_pred=[None] + g["md"]["best_pred"][1:])
        g["cb"] = dict(g["cb"], src=None)
        return dsp.make_md_search_groups([g])

    add("make_md_search_groups", "make_md_search_groups", md_search)
    add("make_md_search_groups[holes]", "make_md_search_groups", md_search_holes)
    add("make_md_search_groups[]", "make_md_search_groups", lambda: dsp.make_md_search_groups([]))

    def intra_fast_search():
        T = Tensors()
        fl = lambda i: dicts(T, **FAST_LOOP)[i]
        return dsp.make_intra_fast_search_groups([dict(luma=fl(0), cb=fl(0), cr=fl(2), pick=dicts(T, **FAST_PICK)[0]),
                                                  dict(luma=fl(1), pick=dicts(T, **FAST_PICK)[1]), dict(luma=fl(2), cb=None, pick=dicts(T, **FAST_PICK)[2])])

    add("make_intra_fast_search_groups", "make_intra_fast_search_groups", intra_fast_search)
    add("make_intra_fast_search_groups[]", "make_intra_fast_search_groups", lambda: dsp.make_intra_fast_search_groups([]))

    def cdef(stack, esize, which):
        T = Tensors()
        rec, other, skip = pic_planes(T, stack, esize), pic_planes(T, stack, esize), T(((3,) if stack else ()) + (6, 10))
        return dsp.make_cdef_pic(rec, skip, 61, 45, 8 if esize == 1 else 10, 37, **{which: other})

    def dlf(stack, esize, which, deltas):
        T = Tensors()
        rec, other, mi = pic_planes(T, stack, esize), pic_planes(T, stack, esize), T(((3,) if stack else ()) + (12, 16, 4))
        kw = dict(ref_deltas=[1, 0, 0, 0, -1, 0, -1, -1], mode_deltas=[2, -2]) if deltas else {}
        return dsp.make_dlf_pic(rec, mi, 61, 45, 8 if esize == 1 else 10, (3, 4, 5, 6), 2, **kw, **{which: other})

    def lr(stack, esize, which, dblk):
        T = Tensors()
        cd, db, other = pic_planes(T, stack, esize), pic_planes(T, stack, esize), pic_planes(T, stack, esize)
        return dsp.make_lr_pic(cd, db if dblk else None, 61, 45, 8 if esize == 1 else 10, (64, 32, 33), **{which: other})

    for stack, esize, which in ((False, 1, "src"), (True, 1, "dst"), (False, 2, "dst"), (True, 2, "src")):
        tag = f"[{'stack' if stack else 'one'}, {8 if esize == 1 else 10} bit, {which}]"
        add("make_cdef_pic" + tag, "make_cdef_pic", lambda a=(stack, esize, which): cdef(*a))
        add("make_dlf_pic" + tag, "make_dlf_pic", lambda a=(stack, esize, which): dlf(*a, deltas=stack))
        add("make_lr_pic" + tag, "make_lr_pic", lambda a=(stack, esize, which): lr(*a, dblk=not stack))
    return c


def uninitialised_dsp(pkg):
    """an SvtHipDsp without a device or a library: the builders need neither"""
    return object.__new__(pkg.SvtHipDsp)


def run_cases(pkg):
    out = {}
    for cid, name, thunk in cases(uninitialised_dsp(pkg)):
        rec = thunk()
        out[cid] = (masked_bytes(rec, MASKED[name]) if name in MASKED else bytes(rec)).hex()
    return out
