"""CPU-only: the Plookup entries (plk_plookup_grand_product[_dev], plk_plookup_vanishing_points[_dev]) are declared in
include/plonky_hip.h, bound in lib.SYMBOLS with the size (c_uint) first, exported by libplonky_hip.so and its checked twin and
wrapped by api / device; the host sort reproduces the reference's sort_by; and the identity the device table rests on,
L_n(x) = L_0(x w) including eval_l_i's zero at its own basis point, holds with integers."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from oracle import bigint_ref as br
from plonky_amd import api, lib
from tests import checked_child
from tests import plookup_ref as pr
from tests.test_oracle_plonk import mont, unmont

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"plk_plookup_grand_product_dev": 10, "plk_plookup_grand_product": 9, "plk_plookup_vanishing_points_dev": 8, "plk_plookup_vanishing_points": 7}


def test_entries_are_declared_and_bound_size_first():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plonky_hip.h")).read(), flags=re.S)
    bound = {name: args for name, _, args in lib.SYMBOLS}
    for name, n_args in NAMES.items():
        assert re.search(r"\bint\s+%s\s*\(\s*unsigned\s+log_size\s*,\s*int\s+field\b" % name, text), name
        assert name in bound, name
        assert len(bound[name]) == n_args and bound[name][0] is ctypes.c_uint and bound[name][1] is ctypes.c_int, name


def test_entries_are_exported():
    lib.build()
    for so in (lib.SO_PATH, checked_child.CHECKED):
        L = ctypes.CDLL(so)
        for name in NAMES:
            assert hasattr(L, name), (so, name)


def test_python_layers_expose_the_functions():
    from plonky_amd import device
    for fn in ("plookup_grand_polynomial", "plookup_vanishing_values", "plookup_sorted_multiset"):
        assert callable(getattr(api, fn)), fn
    for fn in ("plookup_grand_polynomial_dev", "plookup_vanishing_values_dev"):
        assert callable(getattr(device, fn)), fn


def test_sorted_multiset_reproduces_test_sort_by():
    """plookup.rs:297-302: sort_by([5, 2, 1], [1, 2, 3, 4, 5]) = [1, 2, 5].  The helper sorts f ++ t, so the expected multiset is the
    reference's result merged into t in t's order."""
    f = br.TWEEDLEDEE_BASE
    assert pr.sort_by([5, 2, 1], [1, 2, 3, 4, 5]) == [1, 2, 5]
    s = api.plookup_sorted_multiset(mont(f, [5, 2, 1]), mont(f, [1, 2, 3, 4, 5]))
    assert unmont(f, s) == [1, 1, 2, 2, 3, 4, 5, 5]
    assert unmont(f, s) == pr.sort_by([5, 2, 1] + [1, 2, 3, 4, 5], [1, 2, 3, 4, 5])


@pytest.mark.parametrize("f", [br.TWEEDLEDUM_BASE, br.BLS12_377_SCALAR], ids=lambda f: f.name)
def test_sorted_multiset_matches_brute_force(f):
    rng = random.Random(0x50F7 + f.field_id)
    for n_t, n_f in ((8, 7), (64, 63), (33, 200), (16, 0)):
        t = [rng.randrange(f.p) for _ in range(n_t)]
        t[n_t // 2] = t[1]  # a repeated table entry: position() finds the first
        fv = [rng.choice(t) for _ in range(n_f)]
        got = api.plookup_sorted_multiset(mont(f, fv).reshape(-1, 4), mont(f, t))
        assert unmont(f, got) == pr.sort_by(fv + t, t)
    with pytest.raises(AssertionError):
        api.plookup_sorted_multiset(mont(f, [(t[0] + 1) % f.p if (t[0] + 1) % f.p not in t else 7]), mont(f, t))


@pytest.mark.parametrize("f", [br.TWEEDLEDEE_BASE, br.PALLAS_BASE], ids=lambda f: f.name)
@pytest.mark.parametrize("log_size", [1, 2, 5])
def test_last_lagrange_factor_is_the_first_one_shifted(f, log_size):
    """eval_l_i(N, n, w, g4^i) == eval_l_i(N, 0, w, g4^((i + 4) mod 4N)) at every point of the 4N domain, and both are 0 at i = 0 (mod 4)"""
    p, size = f.p, 1 << log_size
    g4 = f.primitive_root_of_unity(log_size + 2)
    w = pow(g4, 4, p)
    xs = [pow(g4, i, p) for i in range(4 * size)]
    l0 = [pr.eval_l_i(f, size, 0, w, x) for x in xs]
    ln = [pr.eval_l_i(f, size, size - 1, w, x) for x in xs]
    assert ln == [l0[(i + 4) % (4 * size)] for i in range(4 * size)]
    assert all(l0[i] == 0 and ln[i] == 0 for i in range(0, 4 * size, 4)) and all(l0[i] != 0 for i in range(4 * size) if i % 4)
