"""An independent restatement of src/hash_to_curve.rs:13-76 (blake_field, blake_hash_base_field_to_curve, blake_hash_usize_to_curve)
in Python integers, for the tests of plonky_amd/csrc/hash_to_curve.hip.

BLAKE3 is restated from its specification for the only case the reference reaches: one block, unkeyed, at most 64 bytes of message
and of extended output (tests/test_hash_to_curve_host_replay.py holds it to three published digests).  The square root is
oracle_lib.field_sqrt, the restatement of Field::square_root that tests/test_oracle_serialization.py pins: the SIGN of the root
matters here, y_neg negates whatever root Tonelli-Shanks returns.  Values are plain integers; (x, y, i, j) says which path a seed took:
i curve tries failed before the one that gave the point, and j hashes of that try were not below the modulus."""
import functools

import numpy as np

from oracle import bigint_ref as br
from oracle import oracle_lib as ol

IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
PERMUTATION = (2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8)
CHUNK_START, CHUNK_END, ROOT = 1, 2, 8
M32 = 0xFFFFFFFF


def _rotr(x, r):
    return ((x >> r) | (x << (32 - r))) & M32


def _g(v, a, b, c, d, mx, my):
    v[a] = (v[a] + v[b] + mx) & M32
    v[d] = _rotr(v[d] ^ v[a], 16)
    v[c] = (v[c] + v[d]) & M32
    v[b] = _rotr(v[b] ^ v[c], 12)
    v[a] = (v[a] + v[b] + my) & M32
    v[d] = _rotr(v[d] ^ v[a], 8)
    v[c] = (v[c] + v[d]) & M32
    v[b] = _rotr(v[b] ^ v[c], 7)


def blake3_xof64(message):
    """the first 64 bytes of the extended output of unkeyed BLAKE3 over a message of at most 64 bytes"""
    message = bytes(message)
    assert len(message) <= 64
    m = [int.from_bytes(message.ljust(64, b"\0")[4 * k:4 * k + 4], "little") for k in range(16)]
    v = list(IV) + list(IV[:4]) + [0, 0, len(message), CHUNK_START | CHUNK_END | ROOT]
    for rnd in range(7):
        _g(v, 0, 4, 8, 12, m[0], m[1])
        _g(v, 1, 5, 9, 13, m[2], m[3])
        _g(v, 2, 6, 10, 14, m[4], m[5])
        _g(v, 3, 7, 11, 15, m[6], m[7])
        _g(v, 0, 5, 10, 15, m[8], m[9])
        _g(v, 1, 6, 11, 12, m[10], m[11])
        _g(v, 2, 7, 8, 13, m[12], m[13])
        _g(v, 3, 4, 9, 14, m[14], m[15])
        m = [m[PERMUTATION[k]] for k in range(16)]
    out = [v[k] ^ v[k + 8] for k in range(8)] + [v[k + 8] ^ IV[k] for k in range(8)]
    return b"".join(w.to_bytes(4, "little") for w in out)


def blake_field(field, iteration, seed):
    """blake_field(iter, seed) over FIELDS[field], seed canonical: (x canonical, y_neg, j)"""
    f = br.FIELDS[field]
    nbytes = 8 * f.n_limbs
    head = int(seed).to_bytes(nbytes, "little") + bytes([iteration])
    for j in range(256):
        container = bytearray(blake3_xof64(head + bytes([j]))[:nbytes + 1])
        container[nbytes - 1] >>= 8 * nbytes - f.bits
        x = int.from_bytes(container[:nbytes], "little")
        if x < f.p:
            return x, container[nbytes] & 1, j
    raise OverflowError("j passed 255")


def _sqrt(f, a):
    """Field::square_root through the oracle: the root the reference returns, or None"""
    r = ol.field_sqrt(f.field_id, np.array(f.mont_limbs(a), dtype=np.uint64))
    return None if r is None else f.from_mont(br.limbs_to_int(r))


@functools.lru_cache(maxsize=None)
def hash_field_to_curve(curve, seed):
    """blake_hash_base_field_to_curve::<C>(seed), seed canonical: (x, y, i, j)"""
    c = br.CURVES[curve]
    f = c.base
    for i in range(256):
        x, y_neg, j = blake_field(f.field_id, i, seed)
        y = _sqrt(f, (x * x * x + c.b) % f.p)
        if y is not None:
            return x, ((f.p - y) % f.p if y_neg else y), i, j
    raise OverflowError("i passed 255")


def hash_usize_to_curve(curve, seed):
    return hash_field_to_curve(curve, int(seed))


def points_mont(curve, seeds):
    """the points of `seeds` as the library stores them: (n, 2, L) Montgomery limbs"""
    f = br.CURVES[curve].base
    out = np.zeros((len(seeds), 2, f.n_limbs), dtype=np.uint64)
    for k, s in enumerate(seeds):
        x, y, _, _ = hash_field_to_curve(curve, int(s))
        out[k, 0] = f.mont_limbs(x)
        out[k, 1] = f.mont_limbs(y)
    return out
