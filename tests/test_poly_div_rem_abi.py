"""CPU-only: the four entry points of the series inverse and the general polynomial division (plk_poly_inv_mod_xn[_dev],
plk_poly_div_rem[_dev]) are declared in include/plonky_hip.h, bound in lib.SYMBOLS with the right argument counts - a size first, the
field id second - and exported by libplonky_hip.so and its checked twin; the api / device wrappers exist; the branches of
api.polynomial_div_rem that need no division launch nothing; and the reference of the GPU tests (tests/poly_newton_ref.py) agrees
with itself."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from plonky_amd import lib
from tests import checked_child
from tests import poly_newton_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG_COUNTS = {"plk_poly_inv_mod_xn_dev": 7, "plk_poly_inv_mod_xn": 5, "plk_poly_div_rem_dev": 10, "plk_poly_div_rem": 8}
P_TWEEDLEDUM_BASE = 0x40000000000000000000000000000000038aa1276c3f59b9a14064e200000001


def _header():
    return open(os.path.join(ROOT, "include", "plonky_hip.h")).read()


def test_entries_are_declared_and_bound_size_first():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    bound = {name: args for name, _, args in lib.SYMBOLS}
    for name, count in ARG_COUNTS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == count, name
        assert params[0].startswith("size_t ") and params[1] == "int field", name
        assert name in bound and len(bound[name]) == count, name
        assert bound[name][0] is ctypes.c_size_t and bound[name][1] is ctypes.c_int, name


def test_entries_are_exported():
    lib.build()
    for so in (lib.SO_PATH, checked_child.CHECKED):
        L = ctypes.CDLL(so)
        for name in ARG_COUNTS:
            assert hasattr(L, name), (so, name)


def test_python_wrappers_exist():
    from plonky_amd import api
    for name in ("polynomial_inv_mod_xn", "polynomial_div_rem", "polynomial_division"):
        assert callable(getattr(api, name)), name
    src = open(os.path.join(ROOT, "plonky_amd", "device.py")).read()  # device.py imports torch: read, do not import
    for name in ("polynomial_inv_mod_xn_dev", "polynomial_div_rem_dev", "polynomial_division_dev"):
        assert re.search(r"^def %s\(" % name, src, flags=re.M), name


def test_branches_without_a_division_launch_nothing(monkeypatch):
    from plonky_amd import api

    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(api._lib, "load", no_library)
    p, fid = P_TWEEDLEDUM_BASE, api.TWEEDLEDUM_BASE
    w = lambda vals: nr.ints_to_words(nr.stored(p, vals))
    big = list(range(1, 41))  # a divisor of degree 39: above the recurrence route's limit
    q, r = api.polynomial_div_rem(fid, w([0, 0, 0]), w(big))  # zero a -> ([0], empty)
    assert nr.words_to_ints(q) == [0] and r.shape == (0, 4)
    a = [3, 4, 0, 9]
    q, r = api.polynomial_div_rem(fid, w(a), w(big))  # deg a < deg b -> ([0], a)
    assert nr.words_to_ints(q) == [0] and nr.words_to_ints(r) == nr.stored(p, a)
    with pytest.raises(ZeroDivisionError):
        api.polynomial_div_rem(fid, w(a), w([0] * 40))
    with pytest.raises(ValueError, match="Inverse doesn't exist"):
        api.polynomial_inv_mod_xn(fid, w([0, 1, 2]), 5)


def test_the_reference_agrees_with_itself():
    p, rng = P_TWEEDLEDUM_BASE, random.Random(1)
    for la, k in ((1, 0), (2, 1), (9, 3), (40, 39), (70, 33), (100, 7)):
        a = nr.rand_poly(p, rng, la)
        b = nr.rand_poly(p, rng, k) + [rng.randrange(1, p)]
        q, r = nr.divide(p, a, b)
        assert len(q) == la - k and len(r) == k
        qb = nr.mul_trunc(p, q, b, la)
        assert [(x + (r[i] if i < k else 0)) % p for i, x in enumerate(qb)] == a
        x = rng.randrange(p)
        assert nr.horner(p, a, x) == (nr.horner(p, q, x) * nr.horner(p, b, x) + nr.horner(p, r, x)) % p
    for n, lh in ((1, 1), (2, 5), (17, 3), (64, 64), (90, 200)):
        h = [rng.randrange(1, p)] + nr.rand_poly(p, rng, lh - 1)
        g = nr.inverse_series(p, h, n)
        assert len(g) == n and nr.mul_trunc(p, g, h, n) == [1] + [0] * (n - 1)
    vals = nr.rand_poly(p, rng, 12)
    assert nr.canonical(p, nr.words_to_ints(nr.ints_to_words(nr.stored(p, vals)))) == vals
    assert np.array_equal(nr.ints_to_words([1, 2 ** 64]), np.array([[1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.uint64))
