"""CPU-only: the grand product Z of the permutation argument (plk_plonk_permutation_z[_dev]) is declared in
include/plonky_hip.h, bound in lib.SYMBOLS and exported by libplonky_hip.so and its checked twin."""
import ctypes
import os
import re

from plonky_amd import lib
from tests import checked_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("plk_plonk_permutation_z_dev", "plk_plonk_permutation_z")


def test_permutation_z_is_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plonky_hip.h")).read(), flags=re.S)
    bound = {name: args for name, _, args in lib.SYMBOLS}
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in bound, name
    assert len(bound["plk_plonk_permutation_z_dev"]) == 11 and len(bound["plk_plonk_permutation_z"]) == 10


def test_permutation_z_is_exported():
    lib.build()
    for so in (lib.SO_PATH, checked_child.CHECKED):
        L = ctypes.CDLL(so)
        for name in NAMES:
            assert hasattr(L, name), (so, name)
