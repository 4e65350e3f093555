"""CPU-only: the three entry points of the low-degree polynomial division (plk_poly_division_dev, plk_poly_division,
plk_poly_from_roots) are declared in include/plonky_hip.h, bound in lib.SYMBOLS with the right argument counts and exported by
libplonky_hip.so and its checked twin; the degree limit of the header is 32; the api / device wrappers exist."""
import ctypes
import os
import re

from plonky_amd import lib
from tests import checked_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG_COUNTS = {"plk_poly_division_dev": 9, "plk_poly_division": 8, "plk_poly_from_roots": 4}


def _header():
    return open(os.path.join(ROOT, "include", "plonky_hip.h")).read()


def test_division_entries_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    bound = {name: args for name, _, args in lib.SYMBOLS}
    for name, count in ARG_COUNTS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == count, name
        assert name in bound and len(bound[name]) == count, name


def test_degree_limit_is_32():
    m = re.search(r"^#define\s+PLK_POLY_DIV_MAX_DEGREE\s+(\d+)\s*$", _header(), flags=re.M)
    assert m and int(m.group(1)) == 32
    from plonky_amd import api
    assert api.POLY_DIV_MAX_DEGREE == 32


def test_division_entries_are_exported():
    lib.build()
    for so in (lib.SO_PATH, checked_child.CHECKED):
        L = ctypes.CDLL(so)
        for name in ARG_COUNTS:
            assert hasattr(L, name), (so, name)


def test_python_wrappers_exist():
    from plonky_amd import api
    for name in ("polynomial_division", "polynomial_long_division", "polynomial_from_roots", "scale_polynomials"):
        assert callable(getattr(api, name)), name
    src = open(os.path.join(ROOT, "plonky_amd", "device.py")).read()  # device.py imports torch: read, do not import
    for name in ("polynomial_division_dev", "public_input_quotient_dev"):
        assert re.search(r"^def %s\(" % name, src, flags=re.M), name
