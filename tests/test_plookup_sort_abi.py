"""CPU-only: the sorted-multiset entries (plk_plookup_sorted_multiset[_dev]) are declared size-first in include/plonky_hip.h, bound in
lib.SYMBOLS with 7 and 6 arguments, exported by libplonky_hip.so and its checked twin, and wrapped by api / device."""
import ctypes
import os
import re

from plonky_amd import api, lib
from tests import checked_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"plk_plookup_sorted_multiset_dev": 7, "plk_plookup_sorted_multiset": 6}


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
    assert callable(getattr(api, "plookup_sorted_multiset_device"))
    assert callable(getattr(device, "plookup_sorted_multiset_dev"))
