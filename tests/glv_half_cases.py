"""Scalars chosen by what their endomorphism halves look like, for the three device paths that recode the halves of glv.cuh's split
(tests/test_gpu_glv_paths.py): the table-free MSM (signed c-bit windows of each half, ord_digit with raw_signed = 1), the pairwise
generator fold and the 2^r-to-1 fold (joint sparse forms of the two halves, fold.hip).  Pure host code on Python integers: the
recodings are restated here from the kernels' comments and loops, the split and the lattice constants come from
tests/scalar_mul_cases.py (which reads glv_params.cuh as data).  tests/test_glv_half_cases.py states what a pool must hold."""
import random
from collections import namedtuple

from oracle import bigint_ref as br
from tests.scalar_mul_cases import GLV_BITS, glv_edge_scalars, glv_params, glv_split

ENDO_CURVES = (0, 1, 3, 4)                # Tweedledee, Tweedledum, Pallas, Vesta
WINDOWS = (3, 4, 7, 10, 12, 13, 16)
PLANT_BITS = 125                          # every K < 2^125 splits into (K, 0) on the four curves
SEARCH_STEP_BITS = 119
SEARCH_STEPS = 1024

Member = namedtuple("Member", "label k k1 k2")


def windows_of(c):
    """windows of a half scalar: GLV_BITS + 1 = 131 bits (msm_geom.h)"""
    return (GLV_BITS + 1 + c - 1) // c


def _walk(mag, c):
    """ord_digit on a magnitude, window by window: (v = window bits + carry in, signed digit, carry out).  v > 2^(c-1) becomes
    v - 2^c with a carry; a magnitude of 0 (v = 0 or v = 2^c) has no entry but keeps its carry."""
    half, out, carry = 1 << (c - 1), [], 0
    for j in range(windows_of(c)):
        v = ((mag >> (c * j)) & ((1 << c) - 1)) + carry
        carry = 1 if v > half else 0
        out.append((v, v - (carry << c), carry))
    assert carry == 0 and mag >> (c * windows_of(c)) == 0, (hex(mag), c)
    return out


def restated_half_digits(h, c):
    """the signed digits of a half scalar h (sign beside the magnitude, raw_signed = 1): one per window, 0 where the device has no entry;
    a negative half flips every digit"""
    sign = -1 if h < 0 else 1
    digits = [sign * d for _, d, _ in _walk(abs(h), c)]
    assert sum(d << (c * j) for j, d in enumerate(digits)) == h
    assert all(abs(d) <= 1 << (c - 1) for d in digits)
    return digits


def half_profile(h, c):
    """what the recoding of |h| goes through: (tie digits v = 2^(c-1), digits -(2^(c-1) - 1): the first negative one, the longest
    run of consecutive windows v = 2^c: no entry, carry kept)"""
    half = 1 << (c - 1)
    ties = near = run = best = 0
    for v, d, carry in _walk(abs(h), c):
        ties += v == half
        near += d == -(half - 1) and carry == 1
        run = run + 1 if v == 1 << c else 0
        best = max(best, run)
    return ties, near, best


def restated_jsf(a, b):
    """Solinas' joint sparse form of two non-negative integers as fold.hip's joint_sparse_form builds it: columns (u0, u1) in
    {-1, 0, 1}^2, least significant first.  Per column: l_i = (k_i + d_i) mod 8; an odd l_i gives u_i = 2 - (l_i mod 4), negated when
    l_i is 3 or 5 and the other l is 2 mod 4; d_i flips when 2 d_i = 1 + u_i; both k_i are halved."""
    assert a >= 0 and b >= 0
    k, d, cols = [a, b], [0, 0], []
    while k[0] or k[1] or d[0] or d[1]:
        l = [(k[i] + d[i]) & 7 for i in (0, 1)]
        u = [0, 0]
        for i in (0, 1):
            if l[i] & 1:
                u[i] = 2 - (l[i] & 3)
                if l[i] in (3, 5) and (l[1 - i] & 3) == 2:
                    u[i] = -u[i]
        for i in (0, 1):
            if 2 * d[i] == 1 + u[i]:
                d[i] = 1 - d[i]
            k[i] >>= 1
        cols.append((u[0], u[1]))
    return cols


# ---- the patterns, as magnitudes ----------------------------------------------------------------------------------------------------
def patterns(c):
    """[(name, magnitude)] over m = windows - 2 windows (at most 126 bits: below the largest K that splits into (K, 0), which k1_plants
    asserts): `tie` - every digit 2^(c-1): v > half is false, the digit stays positive and gives no carry; `near` - window bits
    2^(c-1) + 1, then 2^(c-1) plus the carry, so every digit is -(2^(c-1) - 1), the first negative one, and carries; `chain` -
    2^(c-1) + 1 followed by all-ones windows (each v = 2^c: no entry, the carry runs on) up to bit 125, where the carry ends in the
    highest occupied window; `chainN` - the same chain cut after N all-ones windows (2, 3, half of the windows)."""
    half, w = 1 << (c - 1), windows_of(c)
    m = w - 2
    out = [("tie", sum(half << (c * j) for j in range(m)))]
    out.append(("near", (half + 1) + sum(half << (c * j) for j in range(1, m))))
    out.append(("chain", (1 << PLANT_BITS) - (1 << c) + half + 1))
    for cut in sorted({2, 3, w // 2}):
        out.append(("chain%d" % cut, (1 << (c * (cut + 1))) - (1 << c) + half + 1))
    for name, t in out:
        assert 0 < t < 1 << (PLANT_BITS + 1), (c, name)
    return out


def k1_plants(curve, c):
    """[(label, K)]: every pattern as K itself - the scalar is its own first half, the second is 0"""
    out = []
    for name, t in patterns(c):
        assert glv_split(curve, t) == (t, 0), (curve, c, name)
        out.append(("k1:%s" % name, t))
    return out


def plant_k2(curve, t, sg):
    """a scalar whose second half is sg * t: h1 over the multiples of 2^119, nearest first, until (h1 + sg t lambda) mod r splits into
    (h1, sg t) - the split returns the representative inside one cell of the lattice, so the first half has to be chosen to lie in it.
    -> (k, h1) or None"""
    r, lam = br.CURVES[curve].scalar.p, glv_params(curve)["LAMBDA"]
    for s in range(1, SEARCH_STEPS + 1):
        for h1 in (s << SEARCH_STEP_BITS, -(s << SEARCH_STEP_BITS)):
            k = (h1 + sg * t * lam) % r
            if glv_split(curve, k) == (h1, sg * t):
                return k, h1
    return None


_POOLS = {}


def half_pool(curve, c):
    """the scalars for window c, each with its restated halves and a label: the patterns planted in k1 and in k2 (either sign that the
    split's image holds), the scalars of glv_edge_scalars (longest halves, a zero half), 0, 1, r - 1, lambda, r - lambda, 32 seeded ones"""
    if (curve, c) in _POOLS:
        return _POOLS[(curve, c)]
    r, lam = br.CURVES[curve].scalar.p, glv_params(curve)["LAMBDA"]
    cand = list(k1_plants(curve, c))
    for name, t in patterns(c):
        for sg in (1, -1):
            hit = plant_k2(curve, t, sg)
            if hit:
                cand.append(("k2%s:%s" % ("+" if sg > 0 else "-", name), hit[0]))
    cand += [("edge%d" % i, k) for i, k in enumerate(glv_edge_scalars(curve)[0])]
    cand += [("0", 0), ("1", 1), ("r-1", r - 1), ("lambda", lam), ("r-lambda", r - lam)]
    rng = random.Random(0x61F0 + 97 * curve + c)
    cand += [("rand%d" % i, rng.randrange(r)) for i in range(32)]
    pool = []
    for label, k in cand:
        k1, k2 = glv_split(curve, k)
        assert 0 <= k < r and (k1 + k2 * lam - k) % r == 0 and abs(k1) < 1 << GLV_BITS and abs(k2) < 1 << GLV_BITS, (curve, c, label)
        restated_half_digits(k1, c), restated_half_digits(k2, c)     # their own assertions
        pool.append(Member(label, k, k1, k2))
    _POOLS[(curve, c)] = pool
    return pool


def find(pool, label):
    """the member of that label, or None"""
    return next((m for m in pool if m.label == label), None)


def longest(pool):
    """the member with the longest half"""
    return max(pool, key=lambda m: max(abs(m.k1), abs(m.k2)))


def negative_k2_plant(pool):
    """the carry chain on a negative second half: the whole chain where the split's image holds it (Tweedledum, Vesta), else the longest
    cut of it that it holds (Tweedledee, Pallas: a negative second half stays below |B1|, about 2^90)"""
    hits = [m for m in pool if m.label.startswith("k2-:chain")]
    return find(pool, "k2-:chain") or max(hits, key=lambda m: -m.k2)


FOLD_WINDOW = 4


def fold_scalar_pairs(curve):
    """[(label, a, b)] for out_i = [a] lo_i + [b] hi_i from the pool at c = 4: what the two joint sparse forms of a pair fold can look like
    beside each other (lengths na, nb: test_glv_half_cases.py)"""
    pool = half_pool(curve, FOLD_WINDOW)
    lg, one, zero = longest(pool), find(pool, "1"), find(pool, "0")
    k0, tie, chain, negk2 = find(pool, "edge0"), find(pool, "k2+:tie") or find(pool, "k2-:tie"), find(pool, "k1:chain"), negative_k2_plant(pool)
    assert (one.k, zero.k) == (1, 0) and k0.k2 == 0
    return [("longest x longest", lg.k, lg.k), ("(K, 0) x longest", k0.k, lg.k), ("1 x longest", 1, lg.k), ("longest x 1", lg.k, 1),
            ("%s x %s" % (negk2.label, tie.label), negk2.k, tie.k), ("tie x itself", tie.k, tie.k), ("0 x %s" % chain.label, 0, chain.k)]


def jsf_lengths(curve, a, b):
    """(na, nb) of k_fold_digits with use_glv: the forms of (|a1|, |a2|) and (|b1|, |b2|)"""
    return tuple(len(restated_jsf(*map(abs, glv_split(curve, k)))) for k in (a, b))


def multi_fold_scalars(curve, count, start=0):
    """`count` scalars for the 2^r-to-1 fold from the pool at c = 4, from position `start` of: tie, carry chain, longest halves, the
    carry chain on a negative k2, a (K, 0) split, the tie and the first negative digit in k1 - then the rest of the pool in order"""
    pool = half_pool(curve, FOLD_WINDOW)
    first = [find(pool, "k2+:tie") or find(pool, "k2-:tie"), find(pool, "k1:chain"), longest(pool), negative_k2_plant(pool), find(pool, "edge0"), find(pool, "k1:tie"),
             find(pool, "k1:near")]
    rest = [m for m in pool if m not in first]
    return (first + rest)[start:start + count]
