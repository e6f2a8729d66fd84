"""Every operand of one call in a layout of its own.

A whole-picture call takes several picture operands (source, references, reconstruction, output, skip map, mode-info grid ...), each
with a stride of its own and most with an origin and a pitch between the pictures of a stack.  A test that builds them all with one
helper gives them equal fields, and a kernel or a glue line that reads one operand's field where it means another's passes.  This
module gives every operand of a call fields that no other operand of the call has, and makes the mix-up harmless to run:

  * Layout                     where one plane of one operand sits in its allocation
  * place                      uploads a (padded) plane or a stack of them into a poisoned allocation (tests/poison.py) at a Layout
  * assert_guards_intact       after the call: everything of the allocation that is not the operand still holds the fill
  * Plane / CallSpec           what a call does with each plane: the area, the padding it may touch, which fields it takes
  * distinct_layouts           Layouts for all planes of a CallSpec; it asserts, on the host and before anything is uploaded, that they
                               are PAIRWISE DISTINCT (check_distinct) and SWAP-SAFE (check_swap_safe)

Units: a stride, an origin and a pitch count samples of the plane they belong to (bytes for 8-bit planes, 16-bit words for 10-bit ones,
4-byte records for a mode-info grid), as the calls take them.
"""
import collections
import itertools

import numpy as np

import poison

Layout = collections.namedtuple("Layout", ("stride", "origin_x", "origin_y", "rows_after", "pitch_extra", "lead"), defaults=(0,))
Layout.__doc__ = """stride: samples between two rows.  origin_x / origin_y: where sample (0, 0) of the picture sits, counted from the start the call
is given (start()).  rows_after: spare rows behind the last row the call may touch.  pitch_extra: spare samples between two pictures of a
stack, on top of whole rows.  lead: spare samples of the allocation BEFORE the start the call is given - no field of any call; it is there
so that a smaller origin of another plane (a level-1 origin on a level-0 plane with its wider padding) still lands inside."""


def rows_of(layout, plane):
    return layout.origin_y + plane.height + plane.after[1] + layout.rows_after


def pitch_of(layout, plane):
    """samples between two pictures of a stack (what the call gets as the pitch)"""
    return layout.stride * rows_of(layout, plane) + layout.pitch_extra


class Plane:
    """One plane of one operand of a call.

    name            "ref0.1", "rec.u", "mi" ...; the part before the dot is the operand, which owns the odd-stride rule
    width, height   the picture area in samples
    before, after   (x, y) samples of padding around the area that the call may read or write
    origin          "field": the call takes the allocation's start and origin_x / origin_y;  "pointer": it takes the address of sample
                    (0, 0), so the origin is no field of the call and cannot be mixed up
    stacked         the call takes a pitch for this plane (n_pictures > 1)
    min_origin      the smallest (x, y) the call's validation accepts
    fixed_origin    ((x, y), why): the call's validation forces this origin; the plane is left out of the origin comparison and `why`
                    names the line that forces it
    avoid_origin    origin values that are not to be used (the fixture's own padding, so that a constant in its place shows)
    luma            the name of the luma plane a chroma plane belongs to
    stride_step     strides must be a multiple of it (1 where the call checks pointer alignment only); a value above 1 comes with
                    `stride_why`
    """

    def __init__(self, name, width, height, before=(0, 0), after=(0, 0), origin="pointer", stacked=True, min_origin=None, fixed_origin=None,
                 avoid_origin=(), luma=None, stride_step=1, stride_why=None):
        assert origin in ("field", "pointer") and (stride_step == 1 or stride_why)
        self.name, self.width, self.height, self.before, self.after = name, int(width), int(height), tuple(before), tuple(after)
        self.origin, self.stacked, self.fixed_origin, self.avoid_origin = origin, stacked, fixed_origin, tuple(avoid_origin)
        self.min_origin = tuple(min_origin) if min_origin is not None else self.before
        self.luma, self.stride_step, self.stride_why = luma, stride_step, stride_why

    @property
    def operand(self):
        return self.name.split(".")[0]


class CallSpec:
    def __init__(self, call, planes, n_pictures=1):
        self.call, self.planes, self.n_pictures = call, list(planes), int(n_pictures)
        assert len({p.name for p in self.planes}) == len(self.planes), "plane names must be unique"

    def plane(self, name):
        return next(p for p in self.planes if p.name == name)

    def exceptions(self):
        """[(field, why)] of everything the two properties leave out for this call"""
        out = [(f"{p.name}.origin", p.fixed_origin[1]) for p in self.planes if p.fixed_origin]
        out += [(f"{p.name}.stride", p.stride_why) for p in self.planes if p.stride_step > 1]
        return out


# ---- the two properties -------------------------------------------------------------------------------------------------------------
def _pairs_differ(values, what, call):
    for (na, a), (nb, b) in itertools.combinations(values, 2):
        assert a != b, f"{call}: {what} of {na} and of {nb} are both {a}: a mix-up of the two would not show"


def check_distinct(spec, layouts):
    """PAIRWISE DISTINCT.  Every stride of the call differs from every other; so do the pitches (in a stack) and the origins of the planes
    whose origin is a field of the call and not forced; a chroma stride is neither its luma stride nor half of it; every operand has an odd
    stride where the call takes one; the call's own validation accepts the layout."""
    c = spec.call
    for p in spec.planes:
        l = layouts[p.name]
        assert l.stride % p.stride_step == 0, f"{c}: stride {l.stride} of {p.name} is no multiple of {p.stride_step} ({p.stride_why})"
        assert l.origin_x >= p.min_origin[0] and l.origin_y >= p.min_origin[1], f"{c}: origin of {p.name} below what the call accepts"
        assert l.stride >= l.origin_x + p.width + p.after[0], f"{c}: stride of {p.name} below origin + width + padding"
        assert l.rows_after >= 0 and l.pitch_extra >= 0
        if p.fixed_origin:
            assert (l.origin_x, l.origin_y) == tuple(p.fixed_origin[0]), f"{c}: origin of {p.name} is forced to {p.fixed_origin[0]} ({p.fixed_origin[1]})"
        assert l.origin_x not in p.avoid_origin and l.origin_y not in p.avoid_origin, f"{c}: origin of {p.name} is a value to avoid"
    _pairs_differ([(p.name, layouts[p.name].stride) for p in spec.planes], "stride", c)
    if spec.n_pictures > 1:
        _pairs_differ([(p.name, pitch_of(layouts[p.name], p)) for p in spec.planes if p.stacked], "pitch", c)
    free = [p for p in spec.planes if p.origin == "field" and not p.fixed_origin]
    _pairs_differ([(p.name, layouts[p.name].origin_x) for p in free], "origin_x", c)
    _pairs_differ([(p.name, layouts[p.name].origin_y) for p in free], "origin_y", c)
    for p in free:
        assert layouts[p.name].origin_x != layouts[p.name].origin_y, f"{c}: origin_x and origin_y of {p.name} are equal"
    for p in spec.planes:
        if p.luma:
            s, sl = layouts[p.name].stride, layouts[p.luma].stride
            assert s != sl and s != sl >> 1 and s != (sl + 1) >> 1, f"{c}: chroma stride {s} of {p.name} is its luma stride {sl} or half of it"
    for op in sorted({p.operand for p in spec.planes}):
        mine = [p for p in spec.planes if p.operand == op]
        if any(p.stride_step % 2 for p in mine):
            assert any(layouts[p.name].stride % 2 for p in mine), f"{c}: no stride of operand {op} is odd"


def _size(layout, plane, n_pictures):
    return (n_pictures if plane.stacked else 1) * pitch_of(layout, plane)


def _swap_violation(spec, layouts):
    """the first (plane, needed samples, what) for which another plane's fields lead outside the plane's own allocation, or None"""
    n = spec.n_pictures
    for a in spec.planes:
        la = layouts[a.name]
        size = _size(la, a, n)
        strides = [(p.name, layouts[p.name].stride) for p in spec.planes]
        origins = [(p.name, layouts[p.name].origin_x, layouts[p.name].origin_y) for p in spec.planes if p.origin == "field"] if a.origin == "field" \
            else [(a.name, 0, 0)]
        pitches = [(p.name, pitch_of(layouts[p.name], p)) for p in spec.planes if p.stacked] if n > 1 and a.stacked else [(a.name, 0)]
        base = 0 if a.origin == "field" else la.origin_y * la.stride + la.origin_x          # the pointer the call gets
        for (ns, s), (no, ox, oy), (npi, pitch) in itertools.product(strides, origins, pitches):
            what = f"{spec.call}: {a.name} addressed with the stride of {ns} ({s}), the origin of {no} ({ox}, {oy}) and the pitch of {npi} ({pitch})"
            first = base + (oy - a.before[1]) * s + ox - a.before[0]
            last = base + (n - 1 if a.stacked else 0) * pitch + (oy + a.height + a.after[1] - 1) * s + ox + a.width + a.after[0] - 1
            if first + la.lead < 0:
                return a, first, what + f" starts {-first - la.lead} samples before its allocation"
            if last >= size:
                return a, last + 1, what + f" ends at sample {last} of an allocation of {size}"
    return None


def check_swap_safe(spec, layouts):
    """SWAP-SAFE.  Any plane's pointer with the stride of any plane of the call, the origin of any plane whose origin is a field and the
    pitch of any stacked plane, over the rows and columns the call may touch (the area and its padding) of all pictures, stays inside
    that plane's own allocation: a mix-up gives wrong numbers or a damaged guard, never a fault."""
    v = _swap_violation(spec, layouts)
    assert v is None, "not swap-safe: " + v[2]


def distinct_layouts(spec, layouts=None):
    """{plane name: Layout} for all planes of one call, asserted pairwise distinct and swap-safe.  `layouts`: check these instead of
    producing them (what the producer gives is checked in the same way)."""
    if layouts is None:
        layouts = _produce(spec)
    check_distinct(spec, layouts)
    check_swap_safe(spec, layouts)
    return layouts


def _produce(spec):
    """Deterministic: plane i gets the smallest odd stride above origin + width + padding + 2 i + 1 that no plane has yet and that is
    unrelated to its luma stride, origins counted up from the largest padding any plane of the call has (so that another plane's origin
    still leaves room for this one's padding), and allocations sized up until every swap stays inside."""
    lo_x = max(max(p.before[0], p.min_origin[0]) for p in spec.planes)
    lo_y = max(max(p.before[1], p.min_origin[1]) for p in spec.planes)
    out, used_s, used_x, used_y = {}, set(), set(), set()
    for p in spec.planes:                                      # forced origins first: the free ones keep away from them
        if p.fixed_origin:
            used_x.add(p.fixed_origin[0][0]); used_y.add(p.fixed_origin[0][1])
    for i, p in enumerate(spec.planes):
        if p.fixed_origin:
            ox, oy = p.fixed_origin[0]
        elif p.origin == "field":
            ox = next(v for v in itertools.count(max(lo_x, p.min_origin[0]) + 1 + i) if v not in used_x and v not in p.avoid_origin)
            used_x.add(ox)
            oy = next(v for v in itertools.count(max(lo_y, p.min_origin[1]) + 2 + i) if v not in used_y and v not in p.avoid_origin and v != ox)
            used_y.add(oy)
        else:                                                  # no field of the call: room before the picture, another per plane
            ox, oy = p.before[0] + 3 + 2 * i, p.before[1] + 1 + i
        luma = out[p.luma].stride if p.luma else None
        step = p.stride_step
        s = -(-(ox + p.width + p.after[0] + 2 * i + 1) // step) * step
        while s in used_s or (step % 2 and s % 2 == 0) or (luma is not None and s in (luma, luma >> 1, (luma + 1) >> 1)):
            s += step
        used_s.add(s)
        out[p.name] = Layout(s, ox, oy, 1 + i % 3, 3 + 2 * i)
    for _ in range(200):                                       # size up: pitches only grow, and the plane with the largest needs one picture's extent only
        v = _swap_violation(spec, out)
        if v is not None:
            a, need, what = v
            l = out[a.name]
            if need < 0:                                       # another plane's origin or stride starts before this one: lead in
                out[a.name] = l._replace(lead=-need)
                continue
            n = spec.n_pictures if a.stacked else 1
            more = -(-(need - _size(l, a, spec.n_pictures)) // (n * l.stride))
            out[a.name] = l._replace(rows_after=l.rows_after + max(1, more))
            continue
        seen = {}
        clash = None
        if spec.n_pictures > 1:
            for p in spec.planes:
                if p.stacked and seen.setdefault(pitch_of(out[p.name], p), p.name) != p.name:
                    clash = p.name
        if clash is None:
            return out
        out[clash] = out[clash]._replace(pitch_extra=out[clash].pitch_extra + 1)
    raise AssertionError(f"{spec.call}: no swap-safe allocation sizes found")


# ---- upload and check ----------------------------------------------------------------------------------------------------------------
def place(planes_np, layout, n_pictures=1, fill=None, pad=(0, 0), record=False, device="cuda"):
    """planes_np: one padded plane [h, w] or a stack [n_pictures, h, w] (uint8; uint16 travels as int16 bits; with `record`, a trailing
    axis of 4 bytes that is one 4-byte record per sample), `pad` = (x, y) samples of it that lie before sample (0, 0); for the sizes
    distinct_layouts asserted it is the Plane's area with its `before` and `after` padding (place_plane checks that).
    -> (buffer, view): a poisoned 1-D allocation (poison.tensor: the fill byte everywhere, guards round it) of the lead and n_pictures pitches, and
    the view of planes_np in it - rows `stride` apart, pictures `pitch` apart, sample (0, 0) at the layout's origin.  `fill`: the fill
    byte expected of the running test (checked, not chosen here)."""
    import torch
    a = np.ascontiguousarray(planes_np)
    if record:
        assert a.dtype == np.uint8 and a.shape[-1] == 4
        a = a.view(np.int32)[..., 0]
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    stack = a.ndim == 3
    assert a.ndim in (2, 3) and (a.shape[0] if stack else 1) == n_pictures, "planes_np does not hold n_pictures pictures"
    h, w = a.shape[-2:]
    x0, y0 = layout.origin_x - pad[0], layout.origin_y - pad[1]
    assert x0 >= 0 and y0 >= 0 and x0 + w <= layout.stride, "the padded plane does not fit the layout"
    pitch = layout.stride * (y0 + h + layout.rows_after) + layout.pitch_extra
    dtype = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32}[a.dtype]
    buf = poison.tensor((layout.lead + n_pictures * pitch,), dtype, device)
    assert fill is None or int(buf.view(torch.uint8)[0]) == fill, "the running test's fill byte is not the expected one"
    shape, strides = ((n_pictures,) if stack else ()) + (h, w), ((pitch,) if stack else ()) + (layout.stride, 1)
    view = torch.as_strided(buf, shape, strides, buf.storage_offset() + layout.lead + y0 * layout.stride + x0)
    view.copy_(torch.from_numpy(a).to(device))
    if record:                                                 # back to records: [.., h, w, 4] uint8 over the same bytes
        view = view.view(torch.uint8).unflatten(-1, (w, 4))
    return buf, view


def start(buf, layout):
    """the allocation as the call is to see it: from the sample that origin_x / origin_y count from"""
    return buf[layout.lead:]


def place_plane(plane, planes_np, layout, n_pictures=1, fill=None, record=False, device="cuda"):
    """place() of exactly what the Plane describes: its area with the padding the call may touch"""
    shape = np.shape(planes_np)[-3:-1] if record else np.shape(planes_np)[-2:]
    assert tuple(shape) == (plane.before[1] + plane.height + plane.after[1], plane.before[0] + plane.width + plane.after[0]), (plane.name, shape)
    return place(planes_np, layout, n_pictures, fill, plane.before, record, device)


def sample00(view, plane, record=False):
    """the part of place_plane's view that starts at sample (0, 0): what a call that takes a pointer and no origin gets"""
    return view[..., plane.before[1]:, plane.before[0]:, :] if record else view[..., plane.before[1]:, plane.before[0]:]


def assert_guards_intact(buf, view, fill, what="", content=None):
    """After a call, for an operand from place(), read-only or written: the guards round the allocation (poison.assert_guards) and every
    sample of the allocation outside `view` (the spare columns of each row, the rows before and after, the space between two pictures)
    still hold the fill byte.  content: the numpy plane(s) a read-only operand must still hold."""
    import torch
    poison.assert_guards(buf, fill, what)
    if buf.dtype == torch.int32 and view.dtype == torch.uint8:                     # records
        view = view.flatten(-2).view(torch.int32)
    rest = buf.clone()
    torch.as_strided(rest, view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).view(torch.uint8).fill_(fill)
    bad = (rest.view(torch.uint8) != fill).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} bytes outside the operand were written, the first at byte {int(bad[0])} of the allocation"
    if content is not None:
        want = np.ascontiguousarray(content)
        got = view.cpu().numpy()
        assert np.array_equal(got.view(want.dtype).reshape(want.shape), want), f"{what}: a read-only operand was written"


# ---- the calls -----------------------------------------------------------------------------------------------------------------------
ME_REACH = (66, 32, 16)       # padding round level 0 / 1 / 2 that the ME calls may read: the interpolation's 66 (64 without it), 64 >> level
ME_FIXED_WHY = ("svt_hip_me_frame.hip, me_frame_enqueue: 'the two references' decimated pictures must have the same origin' - one HME "
                "parameter row (pad_width = origin - 1) serves both lists")


def me_spec(call, width, height, n_lists=2, n_pictures=1, me_pads=(68, 34, 17), levels=(0, 1, 2)):
    """src / ref0 / ref1 x pyramid levels.  Origins are fields.  Level 0 of a reference: >= 66 and not the fixture's 68.  Levels 1 and 2 of
    the references stay at the fixture's padding where the whole-picture search runs its HME levels (the named exception)."""
    planes = []
    for k in levels:
        w, h, r = width >> k, height >> k, ME_REACH[k]
        planes.append(Plane(f"src.{k}", w, h, (r, r), (r, r), origin="field", avoid_origin=(me_pads[k],)))
        for l in range(n_lists):
            fixed = ((me_pads[k], me_pads[k]), ME_FIXED_WHY) if k > 0 else None
            planes.append(Plane(f"ref{l}.{k}", w, h, (r, r), (r, r), origin="field", fixed_origin=fixed, avoid_origin=() if fixed else (me_pads[k],)))
    return CallSpec(call, planes, n_pictures)


def picture_spec(call, width, height, operands, n_pictures=1, grid=None):
    """Calls that take (Y, Cb, Cr) pointers with a stride and a pitch per plane (deblocking, CDEF): `operands` names them ("rec", "src",
    "dst"), each with planes .y / .u / .v (4:2:0); grid = (name, unit): one more plane of width / unit x height / unit (the mode-info grid
    in 4-sample units, the skip map in 8-sample units).  Nothing is read outside the picture area, so no plane has padding."""
    planes = []
    for op in operands:
        planes.append(Plane(f"{op}.y", width, height))
        planes += [Plane(f"{op}.{c}", width // 2, height // 2, luma=f"{op}.y") for c in "uv"]
    if grid:
        planes.append(Plane(grid[0], width // grid[1], height // grid[1]))
    return CallSpec(call, planes, n_pictures)


def dlf_spec(call, width, height, operands, n_pictures=1):
    return picture_spec(call, width, height, operands, n_pictures, ("mi", 4))


def cdef_spec(call, width, height, operands, n_pictures=1):
    return picture_spec(call, width, height, operands, n_pictures, ("skip", 8))


def poison_like(a, fill):
    """an array shaped as `a` whose every byte is the fill byte: the content of an output, which the call has to overwrite"""
    return np.full(np.shape(a), fill, np.uint8).astype(np.asarray(a).dtype) * (0x0101 if np.asarray(a).dtype.itemsize == 2 else 1)


def place_operand(spec, lay, operand, contents, n_pictures=1, fill=None, record=False):
    """all planes of one operand, in the spec's order -> (the views from sample (0, 0) on, as a tuple to hand to the call,
    [(plane name, buffer, view, content)] for assert_all_intact)"""
    mine = [p for p in spec.planes if p.operand == operand]
    assert len(mine) == len(contents)
    views, placed = [], []
    for p, c in zip(mine, contents):
        buf, view = place_plane(p, c, lay[p.name], n_pictures, fill, record)
        views.append(sample00(view, p, record))
        placed.append((p.name, buf, view, c))
    return tuple(views), placed


def assert_all_intact(placed, fill, written=False):
    """assert_guards_intact for every plane of place_operand's list; a read-only operand (written = False) also still holds its content"""
    for name, buf, view, content in placed:
        assert_guards_intact(buf, view, fill, name, None if written else content)


def ref_src_spec(call, width, height, pads, operands=("ref", "src")):
    """The inter calls of mode decision: (Y, Cb, Cr) pointers to sample (0, 0) of planes with a border of pads[0] (luma) / pads[1] (chroma)
    samples on every side, a stride per plane and operand, one picture.  Both references share the strides of "ref" (the calls have one
    ref_stride[3] for the two lists), so both are placed at the layouts of "ref"."""
    planes = []
    for op in operands:
        planes.append(Plane(f"{op}.y", width, height, (pads[0],) * 2, (pads[0],) * 2, stacked=False))
        planes += [Plane(f"{op}.{c}", width // 2, height // 2, (pads[1],) * 2, (pads[1],) * 2, stacked=False, luma=f"{op}.y") for c in "uv"]
    return CallSpec(call, planes)


def place_ref_src(spec, lay, planes_np, fill=None):
    """planes_np: {"ref0": [Y, Cb, Cr], "ref1": [..], "src": [..]} padded as ref_src_spec says -> ({name: views at sample (0, 0)},
    {"ref": strides, "src": strides}, placed for assert_all_intact); the six strides are asserted different once more, as the call gets them"""
    P, placed = {}, []
    for n in ("ref0", "ref1", "src"):
        P[n], pl = place_operand(spec, lay, "src" if n == "src" else "ref", planes_np[n], 1, fill)
        placed += [(n + name[3:], b, v, c) for name, b, v, c in pl]
    strides = {op: [lay[f"{op}.{c}"].stride for c in "yuv"] for op in ("ref", "src")}
    assert len(set(strides["ref"] + strides["src"])) == 6
    return P, strides, placed
