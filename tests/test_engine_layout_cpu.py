"""The chunked engine's LDS image (owgs_kernels.hip), read through owgs_engine_lds_regions(_narrow): the
fixed-size regions stand first at offsets that do not depend on the state, the permits, the pool words / usable bitmap and
the bitmap's prefix counts follow.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from openwhisk_amd import _lib

NAMES = ["sc", "ccw", "stgC", "fst", "spt", "hdir", "htab", "hscr", "bhead", "nextl", "spc", "cdirty", "skey", "lq", "fxa",
         "stgX", "stgL", "ct", "stgA", "P", "pool", "pc", "total"]
N_FIXED = NAMES.index("P")  # regions before the permits; the permits' offset is fixed too, their size is not
# uint4 / int4 accesses and LDS-DMA destinations
ALIGN16 = ["ccw", "stgC", "hdir", "lq", "fxa", "stgX", "stgL", "ct", "stgA", "P", "pool", "pc"]
LDS_BYTES = 160 * 1024
# owgs_limits of the parent build (run-time layout, 32-bit cdirty flags): max_invokers, max_slots; and the largest
# identity pool its wide geometry held
PARENT_LIMITS = (20_588, 20_588)
PARENT_WIDE_MAX = 11_024


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    for f in ("owgs_engine_lds_bytes", "owgs_engine_lds_bytes_narrow"):
        getattr(lib, f).restype = C.c_size_t
    return lib


def regions(L, geom, n_slots, pool_mode, n_ids, nm, nb):
    fn = getattr(L, "owgs_engine_lds_regions" + geom)
    out = np.zeros(2 * len(NAMES), np.uint32)
    n = fn(n_slots, pool_mode, n_ids, nm, nb, out.ctypes.data_as(C.c_void_p), len(NAMES))
    assert n == len(NAMES)
    return {k: (int(out[2 * i]), int(out[2 * i + 1])) for i, k in enumerate(NAMES)}


CASES = [(1001, 0, 1001, 901, 100), (1003, 0, 1003, 903, 100), (5000, 0, 5000, 4500, 500), (301, 1, 301, 271, 30),
         (4001, 1, 4001, 3601, 400)]


@pytest.mark.parametrize("geom", ["", "_narrow"])
@pytest.mark.parametrize("case", CASES)
def test_regions_are_disjoint_ordered_and_aligned(L, geom, case):
    r = regions(L, geom, *case)
    end = 0
    for k in NAMES[:-1]:
        off, size = r[k]
        assert off >= end, (k, off, end)
        end = off + size
    assert r["total"][0] >= end and r["total"][0] - end < 16
    assert r["sc"][0] == 0
    for k in ALIGN16:
        assert r[k][0] % 16 == 0, k
    n_slots, pool_mode, n_ids, nm, nb = case
    assert r["P"][1] == 4 * n_slots
    assert r["pool"][1] == (2 * (nm + nb) if pool_mode else 4 * ((n_ids + 31) // 32))
    assert r["pc"][1] == (0 if pool_mode else 4 * ((n_ids + 31) // 32 + 1))
    assert r["total"][0] == getattr(L, "owgs_engine_lds_bytes" + geom)(n_slots, pool_mode, n_ids, nm, nb, 0)


@pytest.mark.parametrize("geom", ["", "_narrow"])
def test_fixed_regions_do_not_move_with_the_state(L, geom):
    ref = regions(L, geom, *CASES[0])
    for case in CASES[1:]:  # other pool sizes, both pool modes
        r = regions(L, geom, *case)
        for k in NAMES[:N_FIXED]:
            assert r[k] == ref[k], k
        assert r["P"][0] == ref["P"][0]
    # the regions every phase touches lie within reach of a ds offset immediate
    for k in ["sc", "ccw", "stgC", "fst", "spt", "hdir", "htab", "hscr", "bhead", "nextl", "spc", "cdirty", "skey", "lq",
              "fxa"]:
        assert ref[k][0] + ref[k][1] <= 65_536, k


def test_limits_and_image_size(L):
    mi, ms = C.c_int32(), C.c_int32()
    assert L.owgs_limits(C.byref(mi), C.byref(ms)) == 0
    assert mi.value >= PARENT_LIMITS[0] and ms.value >= PARENT_LIMITS[1]
    n = mi.value
    assert regions(L, "_narrow", n, 0, n, n, n)["total"][0] <= LDS_BYTES
    assert L.owgs_engine_lds_bytes_narrow(n + 1, 0, n + 1, n + 1, n + 1, 0) > LDS_BYTES
    # the wide geometry holds no less than before either
    n = PARENT_WIDE_MAX
    assert regions(L, "", n, 0, n, n, n)["total"][0] <= LDS_BYTES
