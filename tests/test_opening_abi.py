"""CPU-only: the ten entry points of the opening step (powers, the opened values, the reduced polynomial, halo_b, halo_s; each as a
_dev and a host-pointer form) are declared in include/plonky_hip.h, bound in lib.SYMBOLS with the right argument counts, and
exported by libplonky_hip.so and its checked twin."""
import ctypes
import os
import re

from plonky_amd import lib
from tests import checked_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG_COUNTS = {
    "plk_field_powers_dev": 5, "plk_field_powers": 4,
    "plk_plonk_eval_polys_dev": 8, "plk_plonk_eval_polys": 7,
    "plk_poly_reduce_dev": 8, "plk_poly_reduce": 7,
    "plk_halo_build_b_dev": 7, "plk_halo_build_b": 6,
    "plk_halo_s_dev": 5, "plk_halo_s": 4,
}


def test_opening_entries_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plonky_hip.h")).read(), flags=re.S)
    bound = {name: args for name, _, args in lib.SYMBOLS}
    for name, count in ARG_COUNTS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == count, name
        assert name in bound and len(bound[name]) == count, name


def test_opening_entries_are_exported():
    lib.build()
    for so in (lib.SO_PATH, checked_child.CHECKED):
        L = ctypes.CDLL(so)
        for name in ARG_COUNTS:
            assert hasattr(L, name), (so, name)


def test_python_wrappers_exist():
    from plonky_amd import api
    for name in ("powers", "eval_polys", "reduce_polynomials", "build_halo_b", "halo_s"):
        assert callable(getattr(api, name)), name
