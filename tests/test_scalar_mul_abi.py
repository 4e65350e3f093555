"""CPU-only: the six scalar-multiplication entries (plk_curve_scalar_mul[_dev], plk_halo_n[_dev], plk_halo_n_mul[_dev]) are declared in
include/plonky_hip.h with the argument lists INTEGRATION.md gives - the count first, the curve id second - bound in lib.SYMBOLS,
exported by libplonky_hip.so and its checked twin, wrapped by api / device, and every refusal is PLK_ERR_INVALID_ARG before anything
is launched (so it is seen without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

from plonky_amd import api, lib
from tests import checked_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEAD = r"size_t\s+count\s*,\s*int\s+curve\s*,\s*"
_SC = r"size_t\s+n_scalars\s*,\s*const\s+uint64_t\s*\*\s*scalars\s*,\s*size_t\s+n_points\s*,\s*const\s+uint64_t\s*\*\s*p_xy\s*,\s*const\s+uint8_t\s*\*\s*p_zero\s*,"
_SC += r"\s*uint64_t\s*\*\s*out_xy\s*,\s*uint8_t\s*\*\s*out_zero"
_SCD = r"size_t\s+n_scalars\s*,\s*const\s+void\s*\*\s*d_scalars\s*,\s*size_t\s+n_points\s*,\s*const\s+void\s*\*\s*d_p_xy\s*,\s*const\s+void\s*\*\s*d_p_zero\s*,"
_SCD += r"\s*void\s*\*\s*d_out_xy\s*,\s*void\s*\*\s*d_out_zero\s*,\s*void\s*\*\s*stream"
_BITS = r"unsigned\s+security_bits\s*,\s*"
DECLARATIONS = {
    "plk_curve_scalar_mul": _HEAD + _SC,
    "plk_curve_scalar_mul_dev": _HEAD + _SCD,
    "plk_halo_n": _HEAD + _BITS + r"const\s+uint64_t\s*\*\s*scalars\s*,\s*uint64_t\s*\*\s*out",
    "plk_halo_n_dev": _HEAD + _BITS + r"const\s+void\s*\*\s*d_scalars\s*,\s*void\s*\*\s*d_out\s*,\s*void\s*\*\s*stream",
    "plk_halo_n_mul": _HEAD + _BITS + _SC,
    "plk_halo_n_mul_dev": _HEAD + _BITS + _SCD,
}
N_ARGS = {"plk_curve_scalar_mul": 9, "plk_curve_scalar_mul_dev": 10, "plk_halo_n": 5, "plk_halo_n_dev": 6, "plk_halo_n_mul": 10, "plk_halo_n_mul_dev": 11}
INVALID = lib.PLK_ERR_INVALID_ARG


def test_entries_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plonky_hip.h")).read(), flags=re.S)
    bound = {name: args for name, _, args in lib.SYMBOLS}
    for name, args in DECLARATIONS.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text), name
        assert name in bound and len(bound[name]) == N_ARGS[name], name
        assert bound[name][0] is ctypes.c_size_t and bound[name][1] is ctypes.c_int, name
        if "halo" in name:
            assert bound[name][2] is ctypes.c_uint, name


def test_entries_are_exported_by_both_builds():
    lib.build()
    for so in (lib.SO_PATH, checked_child.CHECKED):
        L = ctypes.CDLL(so)
        for name in DECLARATIONS:
            assert hasattr(L, name), (so, name)


def test_python_layers_expose_the_names():
    from plonky_amd import device
    for name in ("curve_scalar_mul", "halo_n", "halo_n_mul", "halo_g", "schnorr_protocol", "verify_ipa", "verify_halo_g"):
        assert callable(getattr(api, name)), name
    for name in ("scalar_mul_dev", "halo_n_dev", "halo_n_mul_dev"):
        assert callable(getattr(device, name)), name


# ---- refusals: PLK_ERR_INVALID_ARG before anything is launched ----
@pytest.fixture(scope="module")
def L():
    lib.build()
    return lib.load()


BUF = np.zeros(64, dtype=np.uint64)
P = BUF.ctypes.data_as(ctypes.c_void_p)


def mul_calls(L, count=2, curve=0, ns=2, s=P, npts=2, p=P, out=P, oz=P):
    """the four point entries on the same arguments (host pointers stand in for device pointers: a refusal never reads them)"""
    return [L.plk_curve_scalar_mul(count, curve, ns, s, npts, p, None, out, oz),
            L.plk_curve_scalar_mul_dev(count, curve, ns, s, npts, p, None, out, oz, None),
            L.plk_halo_n_mul(count, curve, 128, ns, s, npts, p, None, out, oz),
            L.plk_halo_n_mul_dev(count, curve, 128, ns, s, npts, p, None, out, oz, None)]


def test_unknown_curve_is_refused(L):
    for curve in (-1, 5, 99):
        assert mul_calls(L, curve=curve) == [INVALID] * 4
        assert L.plk_halo_n(2, curve, 128, P, P) == INVALID and L.plk_halo_n_dev(2, curve, 128, P, P, None) == INVALID


def test_null_pointers_are_refused(L):
    for kw in ({"s": None}, {"p": None}, {"out": None}, {"oz": None}):
        assert mul_calls(L, **kw) == [INVALID] * 4, kw
    for s, o in ((None, P), (P, None)):
        assert L.plk_halo_n(2, 0, 128, s, o) == INVALID and L.plk_halo_n_dev(2, 0, 128, s, o, None) == INVALID


def test_broadcast_counts_are_refused_unless_one_or_count(L):
    for kw in ({"count": 4, "ns": 2}, {"count": 4, "npts": 3, "ns": 4}, {"count": 4, "ns": 0, "npts": 4}, {"count": 4, "ns": 4, "npts": 5}):
        assert mul_calls(L, **kw) == [INVALID] * 4, kw


def test_count_of_2_pow_32_is_refused(L):
    big = 1 << 32
    assert mul_calls(L, count=big, ns=big, npts=big) == [INVALID] * 4
    assert mul_calls(L, count=big + 5, ns=1, npts=1) == [INVALID] * 4
    assert L.plk_halo_n(big, 0, 128, P, P) == INVALID and L.plk_halo_n_dev(big, 0, 128, P, P, None) == INVALID


def test_halo_entries_refuse_bls12_377(L):
    assert mul_calls(L, curve=2)[2:] == [INVALID] * 2
    assert L.plk_halo_n(2, 2, 128, P, P) == INVALID and L.plk_halo_n_dev(2, 2, 128, P, P, None) == INVALID
    assert b"endomorphism" in L.plk_last_error()


@pytest.mark.parametrize("bits", (0, 1, 3, 127, 129, 255, 256, 1000))
def test_halo_entries_refuse_bad_security_bits(L, bits):
    for curve in (0, 1, 3, 4):  # ScalarField::BITS = 255: 254 is the largest even number
        assert L.plk_halo_n(2, curve, bits, P, P) == INVALID and L.plk_halo_n_dev(2, curve, bits, P, P, None) == INVALID
        assert L.plk_halo_n_mul(2, curve, bits, 2, P, 2, P, None, P, P) == INVALID
        assert L.plk_halo_n_mul_dev(2, curve, bits, 2, P, 2, P, None, P, P, None) == INVALID


def test_count_zero_is_ok_and_launches_nothing(L):
    assert mul_calls(L, count=0, ns=0, npts=0, s=None, p=None, out=None, oz=None) == [lib.PLK_OK] * 4
    assert L.plk_halo_n(0, 0, 128, None, None) == lib.PLK_OK and L.plk_halo_n_dev(0, 0, 128, None, None, None) == lib.PLK_OK


def test_api_turns_a_refusal_into_value_error():
    with pytest.raises(ValueError):
        api.halo_n(2, np.zeros((1, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        api.halo_n(0, np.zeros((1, 4), dtype=np.uint64), security_bits=7)
