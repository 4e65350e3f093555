"""A restatement of src/hash_to_curve.rs:3-11 and 78-104 (hash_u32_to_curve, hash_usize_to_curve, hash_base_field_to_curve) on Python
integers, for the tests of plonky_amd/csrc/rescue_h2c.hip.  It composes tests/rescue_ref.py (rescue_sponge, and constants: the seeded
stand-in for the reference's round constants) with hash_to_curve_ref._sqrt, the oracle's Field::square_root - the SIGN of the root
matters, y_neg negates whatever root Tonelli-Shanks returns.  security_bits appears as the number of rounds of `consts`.  Values are
canonical integers; (x, y, tries) says how many tries failed before the one that gave the point, which the tests choose inputs by."""
import numpy as np

from oracle import bigint_ref as br
from tests import hash_to_curve_ref as h2c
from tests import rescue_ref as rr

TRIES = 256  # the library's bound on i (H2C_TRIES); the reference loops without one

_cache = {}


def try_outputs(curve, seed, i, consts):
    """rescue_sponge([seed, from_canonical_u32(i)], 2): (x, y_neg)"""
    f = br.CURVES[curve].base
    o = rr.rescue_sponge(f.field_id, [seed % f.p, i], 2, consts)
    return o[0], o[1] & 1  # to_canonical_bool_vec()[0]: bit 0 of limb 0


def hash_base_field_to_curve(curve, seed, consts, key=None, limit=TRIES):
    """hash_base_field_to_curve::<C>(seed, ..), seed canonical: (x, y, tries); None when no i < limit gives a point.
    key: anything hashable that names `consts`, to share results between tests."""
    ck = (curve, seed, key, limit)
    if key is not None and ck in _cache:
        return _cache[ck]
    c = br.CURVES[curve]
    f = c.base
    res = None
    for i in range(limit):
        x, y_neg = try_outputs(curve, seed, i, consts)
        y = h2c._sqrt(f, (x * x * x + c.b) % f.p)
        if y is not None:
            res = (x, (f.p - y) % f.p if y_neg else y, i)
            break
    if key is not None:
        _cache[ck] = res
    return res


def hash_usize_to_curve(curve, seed, consts, key=None):
    return hash_base_field_to_curve(curve, int(seed), consts, key)  # from_canonical_usize: below 2^64, so below every modulus


def hash_u32_to_curve(curve, seed, consts, key=None):
    assert 0 <= seed < 1 << 32
    return hash_base_field_to_curve(curve, int(seed), consts, key)


def points_mont(curve, seeds, consts, key=None):
    """the points of `seeds` as the library stores them, (n, 2, L) Montgomery limbs, and the tries each took"""
    f = br.CURVES[curve].base
    out = np.zeros((len(seeds), 2, f.n_limbs), dtype=np.uint64)
    tries = []
    for k, s in enumerate(seeds):
        x, y, i = hash_base_field_to_curve(curve, int(s), consts, key)
        out[k, 0] = f.mont_limbs(x)
        out[k, 1] = f.mont_limbs(y)
        tries.append(i)
    return out, tries
