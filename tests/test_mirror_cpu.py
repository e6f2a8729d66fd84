"""CPU: the Python mirror against its two sources of truth.

- The make_* builders against tests/golden/mirror_records.json, the bytes the hand-written builders produced before they were folded into
  records.fill / records.build (recorded by tests/golden/make_golden_mirror.py from the commit before the fold; never regenerated).
- signatures.SIGNATURES against the prototypes of include/svt_hip_dsp.h, argument by argument (a device pointer passed as a C int is the
  one segmentation fault this project has had on a GPU), with an entry for every svt_hip_* name the package calls.
- records.RECORDS against the header's structs: one generated C program prints sizeof and every offsetof.

No test here needs the library or a device."""
import ctypes
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mirror_cases  # noqa: E402

HEADER = os.path.join(ROOT, "include", "svt_hip_dsp.h")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "mirror_records.json")))


# -- the builders ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built(pkg):
    """every case built once: {case id: (builder name, the ctypes array or record)}"""
    return {cid: (name, thunk()) for cid, name, thunk in mirror_cases.cases(mirror_cases.uninitialised_dsp(pkg))}


def test_the_case_table_is_the_recorded_one(built):
    assert sorted(built) == sorted(GOLD) and len(GOLD) >= 80


@pytest.mark.parametrize("cid", sorted(GOLD))
def test_builder_bytes_are_the_recorded_ones(built, cid):
    name, rec = built[cid]
    got = (mirror_cases.masked_bytes(rec, mirror_cases.MASKED[name]) if name in mirror_cases.MASKED else bytes(rec)).hex()
    want = GOLD[cid]
    assert len(got) == len(want), (len(got) // 2, len(want) // 2)
    diff = [i // 2 for i in range(0, len(got), 2) if got[i:i + 2] != want[i:i + 2]]
    assert not diff, f"{len(diff)} bytes differ, the first at offset {diff[0]}"


def test_host_addresses_are_set_when_given_and_null_when_not(built):
    """the fields the byte comparison masks"""
    for cid, (name, rec) in built.items():
        if name == "make_recon_final_args":
            given = not any(v in cid for v in ("no groups", "min"))
            assert bool(rec.groups) == given, cid
            assert not given or rec.groups == ctypes.addressof(rec._groups), cid
        elif name == "make_intra_encode_args":
            assert bool(rec.q_luma) == ("min" not in cid) and bool(rec.q_chroma) == ("min" not in cid and "luma rows" not in cid), cid
            if rec.q_luma and rec.q_chroma:
                assert rec.q_luma != rec.q_chroma
                q = ctypes.cast(rec.q_chroma, ctypes.POINTER(type(rec._keep[0]))).contents
                assert ctypes.cast(q.dequant, ctypes.POINTER(ctypes.c_int16))[1] == mirror_cases.QROW_B["dequant"][1]


REQUIRED = (("make_frame_groups", dict(tensors=("xy",), scalars=("src_stride", "pred_stride", "recon_stride", "tx_size", "tx_type"),
                                       required=("src_stride", "pred_stride", "recon_stride", "xy", "tx_size", "tx_type"))),
            ("make_full_loop_groups", mirror_cases.FULL_LOOP), ("make_tx_search_groups", mirror_cases.TX_SEARCH),
            ("make_cfl_search_groups", mirror_cases.CFL_SEARCH), ("make_cfl_pick_groups", mirror_cases.CFL_SEARCH),
            ("make_fast_loop_groups", mirror_cases.FAST_LOOP), ("make_md_decide_groups", mirror_cases.MD_DECIDE))


@pytest.mark.parametrize("name,spec", REQUIRED, ids=[n for n, _ in REQUIRED])
def test_a_missing_required_key_is_a_key_error(pkg, name, spec):
    make = getattr(mirror_cases.uninitialised_dsp(pkg), name)
    minimal = mirror_cases.dicts(mirror_cases.Tensors(), **spec)[1]
    make([minimal])
    for key in spec["required"]:
        with pytest.raises(KeyError):
            make([{k: v for k, v in minimal.items() if k != key}])
    dsp = mirror_cases.uninitialised_dsp(pkg)
    for make, a in ((dsp.make_partition_args, {}), (dsp.make_recon_final_args, {"final_count": mirror_cases.Tensors()()}),
                    (dsp.make_intra_encode_args, {"sb_cols": 1}), (dsp.make_md_search_groups, [{"md": minimal}]),
                    (dsp.make_intra_fast_search_groups, [{"pick": {}}])):
        with pytest.raises(KeyError):
            make(a)


def test_an_empty_list_gives_one_zeroed_record(pkg):
    dsp = mirror_cases.uninitialised_dsp(pkg)
    names = [n for n in dir(dsp) if n.startswith("make_") and n.endswith("_groups")] + ["make_frame_levels"]
    assert len(names) >= 23
    for n in names:
        arr = getattr(dsp, n)([])
        assert len(arr) == (0 if n == "make_frame_groups" else 1) and not any(bytes(arr)), n      # (encode_recon_frame passes len(array) on)


def test_every_name_is_a_module_name_and_a_class_attribute(pkg):
    for cname, rec in pkg.records.RECORDS.items():
        assert getattr(pkg, rec.__name__) is rec and rec.c_name == cname
    for n in pkg.records.DSP_ATTRIBUTES:
        assert getattr(pkg.SvtHipDsp, n) is getattr(pkg, n) is getattr(pkg.records, n), n
    assert pkg.TxDecision is pkg.SvtHipDsp.TxDecision and pkg.MdSearchGroup._fields_[1][1] is pkg.SvtHipDsp.TxSearchGroup
    assert callable(pkg.SvtHipDsp.pack_fast_rates) and pkg.md_decision_dtype().itemsize == 72
    assert not {"build", "fill"} & set(pkg.records.__all__)          # (the package has a submodule named build)


# -- the signatures ----------------------------------------------------------------------------------------------------------------------
def header_text():
    """the header without comments, preprocessor lines and the bodies of structs and enums"""
    s = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    s = re.sub(r"//[^\n]*", " ", s)
    s = "\n".join(l for l in s.split("\n") if not l.lstrip().startswith("#")).replace('extern "C" {', " ")
    while True:
        s, n = re.subn(r"\{[^{}]*\}", " ", s)
        if not n:
            return s


def prototypes():
    """{name: (return type text, [argument text])} of every svt_hip_* function the header declares"""
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(svt_hip_\w+)\s*\(([^()]*)\)\s*;", header_text()):
        args = [a.strip() for a in args.split(",")]
        out[name] = (" ".join(ret.split()), [] if args == ["void"] else args)
    return out


C_INTS = {"int": ("i", 32), "int32_t": ("i", 32), "unsigned": ("u", 32), "uint32_t": ("u", 32), "int16_t": ("i", 16), "uint16_t": ("u", 16),
          "int8_t": ("i", 8), "uint8_t": ("u", 8), "int64_t": ("i", 64), "uint64_t": ("u", 64), "size_t": ("u", 64)}


def c_class(text, is_return=False):
    """the class of a C parameter or return type: "ptr", ("i" | "u", bits), or None for void"""
    if "*" in text or "[" in text:
        return "ptr"
    words = [w for w in text.split() if w != "const"]
    if not is_return and len(words) > 1:
        words = words[:-1]                                   # the parameter's name
    if words == ["void"]:
        return None
    assert len(words) == 1 and words[0] in C_INTS, f"a C type this test does not know: {text!r}"
    return C_INTS[words[0]]


def ctypes_class(t):
    if t is None:
        return None
    code = getattr(t, "_type_", None)
    if t in (ctypes.c_void_p, ctypes.c_char_p) or not isinstance(code, str):
        return "ptr"
    assert code in "bhilqBHILQ", t
    return ("i" if code.islower() else "u", 8 * ctypes.sizeof(t))


def test_the_header_parser_finds_the_prototypes():
    protos = prototypes()
    assert len(protos) >= 180, len(protos)
    assert protos["svt_hip_last_error"] == ("const char *", []) and protos["svt_hip_malloc"][0] == "void *"
    assert c_class("const svt_hip_md_search_group *groups") == "ptr" and c_class("size_t scratch_bytes") == ("u", 64)
    assert c_class("const uint32_t unit_size[3]") == "ptr" and c_class("int16_t search_w") == ("i", 16) and c_class("void", True) is None
    assert ctypes_class(ctypes.c_size_t) == ("u", 64) and ctypes_class(ctypes.c_int) == ("i", 32) and ctypes_class(ctypes.c_char_p) == "ptr"
    assert ctypes_class(ctypes.POINTER(ctypes.c_int)) == "ptr" and ctypes_class(ctypes.c_int64) == ("i", 64)


def test_every_signature_matches_its_prototype(pkg):
    protos, bad = prototypes(), []
    for name, (restype, argtypes) in pkg.signatures.SIGNATURES.items():
        if name not in protos:
            bad.append(f"{name}: no prototype in the header")
            continue
        ret, args = protos[name]
        if ctypes_class(restype) != c_class(ret, True):
            bad.append(f"{name}: returns {ret!r}, restype {restype}")
        if len(args) != len(argtypes):
            bad.append(f"{name}: {len(args)} parameters, {len(argtypes)} argtypes")
            continue
        bad += [f"{name}: parameter {i} is {a!r}, argtype {t}" for i, (a, t) in enumerate(zip(args, argtypes)) if c_class(a) != ctypes_class(t)]
    assert not bad, "\n".join(bad)
    assert len(pkg.signatures.SIGNATURES) >= 147


def test_every_called_name_has_a_signature(pkg):
    """and no wrapper assigns argtypes or restype of its own any more"""
    called = set()
    for path in glob.glob(os.path.join(pkg.PKG_DIR, "*.py")):
        text = open(path).read()
        called |= set(re.findall(r"(?:\blib|\bL|load_library\(\))\.(svt_hip_\w+)", text))
        if not path.endswith("signatures.py"):
            assert not re.search(r"\.(argtypes|restype)\s*=", text), path
    assert len(called) >= 120 and{"svt_hip_init", "svt_hip_lr_unit_offset", "svt_hip_membw_probe_chain"} <= called
    assert not called - set(pkg.signatures.SIGNATURES), sorted(called - set(pkg.signatures.SIGNATURES))


def test_a_missing_symbol_is_an_error_at_load(pkg):
    class Lib:
        def __getattr__(self, name):
            if name == "svt_hip_md_search_frame":
                raise AttributeError(name)
            return type("F", (), {})()

    with pytest.raises(AttributeError, match="svt_hip_md_search_frame"):
        pkg.signatures.apply(Lib())
    with pytest.raises(pkg.SvtHipError):
        pkg.load_library(os.path.join(ROOT, "no", "such", "libsvt_hip_dsp.so"))


# -- the records -------------------------------------------------------------------------------------------------------------------------
def test_every_record_matches_the_header(pkg):
    R = pkg.records
    lines, want = [], []
    for cname, rec in R.RECORDS.items():
        fields = [n for n, _ in rec._fields_]
        exprs = [f"sizeof({cname})", f"_Alignof({cname})"] + [f"offsetof({cname}, {R.C_FIELD.get(n, n)})" for n in fields] + \
                [f"sizeof((({cname} *)0)->{R.C_FIELD.get(n, n)})" for n in fields]
        lines.append('printf("' + " ".join(["%zu"] * len(exprs)) + '\\n", ' + ", ".join(exprs) + ");")
        want.append([ctypes.sizeof(rec), ctypes.alignment(rec)] + [getattr(rec, n).offset for n in fields] + [getattr(rec, n).size for n in fields])
    assert len(want) >= 60
    code = '#include <stddef.h>\n#include <stdio.h>\n#include "svt_hip_dsp.h"\nint main(void)\n{\n' + "\n".join(lines) + "\nreturn 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(code)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [[int(v) for v in l.split()] for l in subprocess.check_output([os.path.join(d, "t")]).decode().splitlines()]
    for (cname, rec), g, w in zip(R.RECORDS.items(), got, want):
        assert g == w, f"{cname} / {rec.__name__}: the header says {g}, ctypes says {w} (sizeof, alignment, offsets, field sizes)"
    assert len(got) == len(want)


def test_the_sizes_the_device_code_relies_on(pkg):
    sizes = {"TxDecision": 40, "MdDecision": 72, "CflDecision": 32, "InterpDecision": 32, "InterBlk": 16, "InterCand": 16, "InterFastBlk": 16,
             "BlkGeom": 16, "WarpSamples": 132, "WarpModel": 36, "MeFrameParams": 116, "MePyramid": 88, "FastLoopGroup": 216, "CdefPic": 232, "MdBlk": 4}
    for n, size in sizes.items():
        assert ctypes.sizeof(getattr(pkg, n)) == size, n
    for n in ("TxDecision", "MdDecision", "CflDecision", "InterpDecision"):
        assert ctypes.alignment(getattr(pkg, n)) == 8, n
    import numpy as np
    for n, dt in (("TxDecision", pkg.TX_DECISION_DTYPE), ("CflDecision", pkg.CFL_DECISION_DTYPE), ("MdDecision", pkg.md_decision_dtype()),
                  ("MdBlk", pkg.md_blk_dtype()), ("InterBlk", pkg.inter_blk_dtype()), ("InterCand", pkg.inter_cand_dtype()),
                  ("InterFastBlk", pkg.inter_fast_blk_dtype()), ("InterpDecision", pkg.interp_decision_dtype()),
                  ("WarpSamples", pkg.warp_samples_dtype()), ("WarpModel", pkg.warp_model_dtype())):
        dt, rec = np.dtype(dt), getattr(pkg, n)
        assert dt.itemsize == ctypes.sizeof(rec) and [(f, dt.fields[f][1]) for f in dt.names] == [(f, getattr(rec, f).offset) for f, _ in rec._fields_], n
