"""CPU-only: the four entries of the Rescue hash to the curve (plk_rescue_hash_to_curve[_dev], plk_rescue_hash_field_to_curve[_dev]) are
declared in include/plonky_hip.h with the argument lists INTEGRATION.md gives - count first, context second: none joins the pinned
id-first set - bound in lib.SYMBOLS, exported by libplonky_hip.so and its checked twin, and wrapped by api / device.  The restatement
tests/rescue_h2c_ref.py is held to what integers alone can say about it."""
import ctypes
import os
import re

import pytest

from oracle import bigint_ref as br
from plonky_amd import api, lib
from tests import checked_child
from tests import rescue_h2c_ref as ref
from tests import rescue_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEAD = r"size_t\s+count\s*,\s*const\s+plk_rescue_ctx\s*\*\s*ctx\s*,\s*int\s+curve\s*,\s*"
DECLARATIONS = {
    "plk_rescue_hash_to_curve": _HEAD + r"uint64_t\s+seed_start\s*,\s*uint64_t\s*\*\s*out_xy",
    "plk_rescue_hash_to_curve_dev": _HEAD + r"uint64_t\s+seed_start\s*,\s*void\s*\*\s*d_out_xy\s*,\s*void\s*\*\s*stream",
    "plk_rescue_hash_field_to_curve": _HEAD + r"const\s+uint64_t\s*\*\s*seeds\s*,\s*uint64_t\s*\*\s*out_xy",
    "plk_rescue_hash_field_to_curve_dev": _HEAD + r"const\s+void\s*\*\s*d_seeds\s*,\s*void\s*\*\s*d_out_xy\s*,\s*void\s*\*\s*stream",
}
N_ARGS = {"plk_rescue_hash_to_curve": 5, "plk_rescue_hash_to_curve_dev": 6, "plk_rescue_hash_field_to_curve": 5, "plk_rescue_hash_field_to_curve_dev": 6}


def test_entries_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plonky_hip.h")).read(), flags=re.S)
    bound = {name: args for name, _, args in lib.SYMBOLS}
    for name, args in DECLARATIONS.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text), name
        assert name in bound and len(bound[name]) == N_ARGS[name], name
        assert bound[name][0] is ctypes.c_size_t and bound[name][1] is ctypes.c_void_p and bound[name][2] is ctypes.c_int, name
    for name in ("plk_rescue_hash_to_curve", "plk_rescue_hash_to_curve_dev"):
        assert bound[name][3] is ctypes.c_uint64, name


def test_entries_are_exported_by_both_builds():
    lib.build()
    for so in (lib.SO_PATH, checked_child.CHECKED):
        L = ctypes.CDLL(so)
        for name in DECLARATIONS:
            assert hasattr(L, name), (so, name)


def test_python_layers_expose_the_reference_names():
    from plonky_amd import device
    for name in ("hash_base_field_to_curve", "hash_u32_to_curve", "hash_usize_to_curve"):
        assert callable(getattr(api, name)), name
    for name in ("rescue_hash_to_curve_dev", "rescue_hash_field_to_curve_dev"):
        assert callable(getattr(device, name)), name
    with pytest.raises(ValueError):  # a u32 seed is a u32: refused before the library is reached
        api.hash_u32_to_curve(None, 0, 1 << 32)
    with pytest.raises(ValueError):
        api.hash_u32_to_curve(None, 0, (1 << 32) - 2, 3)


# ---- the restatement against integers alone ----
@pytest.mark.parametrize("curve", sorted(br.CURVES))
def test_ref_point_is_on_the_curve_with_the_sponge_s_x_and_sign(curve):
    from oracle import oracle_lib as ol
    ol.build()
    c = br.CURVES[curve]
    f = c.base
    rounds = 2
    consts = rr.constants(f.field_id, 4, rounds)
    signs, tries = set(), []
    for seed in [0, 1, 2, 3, 4, 5, 6, 7, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, f.p - 1]:
        x, y, t = ref.hash_base_field_to_curve(curve, seed, consts)
        assert (y * y - x * x * x - c.b) % f.p == 0 and 0 <= x < f.p and 0 < y < f.p
        # x is the sponge's first output at the try that settled, and every earlier try's x has no point
        out = rr.rescue_sponge(f.field_id, [seed, t], 2, consts)
        assert x == out[0]
        for i in range(t):
            xi = rr.rescue_sponge(f.field_id, [seed, i], 2, consts)[0]
            assert pow((xi ** 3 + c.b) % f.p, (f.p - 1) // 2, f.p) == f.p - 1, (seed, i)
        # the sign of y follows bit 0 of the second output: y is the oracle's root, or its negative
        root = ref.h2c._sqrt(f, (x ** 3 + c.b) % f.p)
        assert y == ((f.p - root) % f.p if out[1] & 1 else root)
        signs.add(out[1] & 1)
        tries.append(t)
        if seed < 1 << 64:
            assert ref.hash_usize_to_curve(curve, seed, consts) == (x, y, t)
    assert signs == {0, 1} and max(tries) >= 1 and min(tries) == 0
    assert ref.hash_u32_to_curve(curve, 5, consts) == ref.hash_base_field_to_curve(curve, 5, consts)


def test_ref_seed_and_constants_change_the_point():
    curve, fid = 0, 0
    consts = rr.constants(fid, 4, 2)
    base = ref.hash_base_field_to_curve(curve, 11, consts)
    assert ref.hash_base_field_to_curve(curve, 12, consts)[:2] != base[:2]
    assert ref.hash_base_field_to_curve(curve, 11, rr.constants(fid, 4, 2, seed=1338))[:2] != base[:2]
    p = br.FIELDS[fid].p
    bumped = [(list(a), list(b)) for a, b in consts]
    bumped[0][0][2] = (bumped[0][0][2] + 1) % p  # one constant of the first step, on an element the chunk does not touch
    assert ref.hash_base_field_to_curve(curve, 11, bumped)[:2] != base[:2]
    last = [(list(a), list(b)) for a, b in consts]
    last[1][1][3] = (last[1][1][3] + 1) % p  # the last step's constant of state[3], which is not squeezed: the same point
    assert ref.hash_base_field_to_curve(curve, 11, last) == base
    assert ref.hash_base_field_to_curve(curve, 11, rr.constants(fid, 4, 3))[:2] != base[:2]  # security_bits: the number of rounds
    assert ref.hash_base_field_to_curve(curve, 11, consts, limit=0) is None
