"""CPU-only: the five entries of the BLAKE3 hash to the curve (plk_hash_to_curve[_dev], plk_hash_field_to_curve[_dev], plk_blake_field)
are declared in include/plonky_hip.h count first and id second (the id-first entries are a pinned set), with the argument lists
INTEGRATION.md gives, bound in lib.SYMBOLS, exported by libplonky_hip.so
and its checked twin, and wrapped by api / device under the reference's names."""
import ctypes
import os
import re

from plonky_amd import api, lib
from tests import checked_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARATIONS = {
    "plk_hash_to_curve": r"size_t\s+count\s*,\s*int\s+curve\s*,\s*uint64_t\s+seed_start\s*,\s*uint64_t\s*\*\s*out_xy",
    "plk_hash_to_curve_dev": r"size_t\s+count\s*,\s*int\s+curve\s*,\s*uint64_t\s+seed_start\s*,\s*void\s*\*\s*d_out_xy\s*,\s*void\s*\*\s*stream",
    "plk_hash_field_to_curve": r"size_t\s+count\s*,\s*int\s+curve\s*,\s*const\s+uint64_t\s*\*\s*seeds\s*,\s*uint64_t\s*\*\s*out_xy",
    "plk_hash_field_to_curve_dev": r"size_t\s+count\s*,\s*int\s+curve\s*,\s*const\s+void\s*\*\s*d_seeds\s*,\s*void\s*\*\s*d_out_xy\s*,\s*void\s*\*\s*stream",
    "plk_blake_field": r"size_t\s+count\s*,\s*int\s+field\s*,\s*const\s+uint8_t\s*\*\s*iters\s*,\s*const\s+uint64_t\s*\*\s*seeds\s*,\s*uint64_t\s*\*\s*out_x\s*,"
                       r"\s*uint8_t\s*\*\s*out_y_neg",
}
N_ARGS = {"plk_hash_to_curve": 4, "plk_hash_to_curve_dev": 5, "plk_hash_field_to_curve": 4, "plk_hash_field_to_curve_dev": 5, "plk_blake_field": 6}


def test_entries_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plonky_hip.h")).read(), flags=re.S)
    bound = {name: args for name, _, args in lib.SYMBOLS}
    for name, args in DECLARATIONS.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text), name
        assert name in bound and len(bound[name]) == N_ARGS[name] and bound[name][0] is ctypes.c_size_t and bound[name][1] is ctypes.c_int, name
    for name in ("plk_hash_to_curve", "plk_hash_to_curve_dev"):
        assert bound[name][2] is ctypes.c_uint64, name  # the seed is 64 bits wide on every platform


def test_entries_are_exported_by_both_builds():
    lib.build()
    for so in (lib.SO_PATH, checked_child.CHECKED):
        L = ctypes.CDLL(so)
        for name in DECLARATIONS:
            assert hasattr(L, name), (so, name)


def test_python_layers_expose_the_reference_names():
    from plonky_amd import device
    for name in ("blake_field", "blake_hash_base_field_to_curve", "blake_hash_usize_to_curve", "pedersen_generators"):
        assert callable(getattr(api, name)), name
    assert callable(getattr(device, "hash_to_curve_dev"))
