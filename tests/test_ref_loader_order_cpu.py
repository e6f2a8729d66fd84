"""CPU: the live-reference loaders of the fixture generators (make_golden_cdef / _coeff_rate / _cfl_search .ref_lib) give a usable
library in whatever order they and ref_ois_setup() run.

ref_ois_setup() - run once per process by every ref_ois_* / ref_pins_* / ref_intra_* entry of oracle/_ref/libsvtref.so - refills every
dispatch global with the reference's setup_rtcd_internal(ASM_AVX2); the kernels it names that are not in the compiled source subset
leave their slot NULL.  A loader that pointed its slots once and cached the handle therefore handed out NULL slots after the first
such entry had run: a whole-suite run ended in a segmentation fault inside cdef_filter_fb.  Each order runs in a fresh child process,
so that a crash is a failed assertion carrying the exit status (-11) and not the end of the run."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")

CHILD = r'''
import ctypes, os, sys
import numpy as np
root, order = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(root, "tests"), os.path.join(root, "tests", "golden")]
import make_golden_cdef as cd, make_golden_coeff_rate as cr, make_golden_cfl_search as cf

SLOTS = {cd: ("cdef_find_dir", "cdef_filter_block", "copy_rect8_8bit_to_16bit", "dist_8x8_16bit", "mse_4x4_16bit"),
         cr: ("av1_txb_init_levels", "av1_get_nz_map_contexts"), cf: ("av1_txb_init_levels", "av1_get_nz_map_contexts")}
seen = []


def load():
    """every loader; what each slot it names holds when it returns"""
    libs = {}
    for m, names in SLOTS.items():
        libs[m] = m.ref_lib()
        seen.append((m.__name__, {n: ctypes.c_void_p.in_dll(libs[m], n).value for n in names}))
    return libs


def setup():
    L = ctypes.CDLL(os.path.join(root, "oracle", "_ref", "libsvtref.so"))
    L.ref_ois_setup.restype = None
    L.ref_ois_setup()


if order == "loader_setup_loader":
    load(); setup(); libs = load()
else:
    setup(); libs = load()
print("slots", seen, flush=True)

# one filter block of the CDEF strength search through the reference (fixture case h: 64 x 64, one filter block)
g = np.load(os.path.join(root, "tests", "golden", "cdef.npz"))
bd, w, h, q = (int(v) for v in g["h_meta"])
rec = [g["h_rec_" + c] for c in "yuv"]
src16 = [np.ascontiguousarray(g["h_src_" + c].astype(np.uint16)) for c in "yuv"]
mse, count = cd.ref_search_fb(libs[cd], rec, src16, g["h_skip"], 0, 0, bd, q)[:2]
assert np.array_equal(mse, g["h_mse"][:, 0]) and count == int(g["h_count"][0]), "cdef case h"
print("cdef ok", flush=True)

# one coefficient-rate fixture case (TX_4X4: every block, every transform type) through the reference's av1_cost_coeffs_txb
z = np.load(os.path.join(root, "tests", "golden", "coeff_rate.npz"))
for k, v in cr.gen_size(0, libs[cr]).items():
    assert np.array_equal(v, z["s0_" + k]), ("coeff_rate s0", k)
print("coeff_rate ok", flush=True)

# a NULL slot that something above called has ended this process already; one that nothing called fails here
for name, slots in seen:
    assert all(slots.values()), (name, slots)
print("all ok", flush=True)
'''


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/libsvtref.so is not built here (it needs the reference's sources)")
@pytest.mark.parametrize("order", ["loader_setup_loader", "setup_loader"])
def test_the_loaders_give_a_usable_reference_in_either_order(order):
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, order], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("all ok"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
