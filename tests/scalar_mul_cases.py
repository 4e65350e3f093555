"""Cases of the scalar-multiplication tests (tests/test_gpu_scalar_mul.py, in process and through the checked build): (scalar, point)
pairs on Python integers, their packing into the interface's arrays and the comparison with oracle.bigint_ref.ec_mul, limb for limb."""
import numpy as np

from oracle import bigint_ref as br
from tests import halo_endo_ref as he


def edge_scalars(curve):
    c = br.CURVES[curve]
    r = c.scalar.p
    out = [0, 1, 2, 3, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2]
    # 2^k and 2^k - 1 at the digit (2 bits), word (32), limb (64) and half (GLV_BITS = 130) boundaries and at the top
    for k in (2, 3, 31, 32, 33, 64, 65, 127, 128, 129, 130, 131, 192, c.scalar.bits - 2, c.scalar.bits - 1):
        out += [(1 << k) % r, ((1 << k) - 1) % r]
    if curve in he.ENDO_CURVES:
        lam = he.zeta_scalar(curve)
        out += [lam, (lam + 1) % r, lam - 1, r - lam, lam * lam % r]
        out += glv_edge_scalars(curve)[0]  # chosen with the restated split: a zero half beside the longest other half, the longest halves
    return out


def random_scalars(curve, seed, count):
    f = br.CURVES[curve].scalar
    return [br.limbs_to_int(l) % f.p for l in br.rand_field_limbs(f, seed, count)]


def base_points(curve):
    """G, 2G, a seeded multiple, -G and the identity"""
    c = br.CURVES[curve]
    G = (c.gx, c.gy)
    return [G, br.ec_add(c, G, G), br.ec_mul(c, 0x5EEDED + curve, G), br.ec_neg(c, G), None]


def pairs(curve, extra_points=()):
    """every edge scalar and 64 seeded ones on G, and the same scalars dealt round over the other points"""
    pts = base_points(curve) + list(extra_points)
    scalars = edge_scalars(curve) + random_scalars(curve, 77 + curve, 64)
    out = [(s, pts[0]) for s in scalars]
    out += [(s, pts[1 + i % (len(pts) - 1)]) for i, s in enumerate(scalars)]
    return out


def pack(curve, prs):
    c = br.CURVES[curve]
    L = c.base.n_limbs
    s = np.array([c.scalar.mont_limbs(k) for k, _ in prs], dtype=np.uint64).reshape(-1, 4)
    p = np.zeros((len(prs), 2, L), dtype=np.uint64)
    z = np.zeros(len(prs), dtype=np.uint8)
    for i, (_, P) in enumerate(prs):
        if P is None:
            z[i] = 1
            p[i] = 0xDEAD  # the coordinates of a flagged point are not read as a point
        else:
            p[i] = [c.base.mont_limbs(P[0]), c.base.mont_limbs(P[1])]
    return s, p, z


def point_limbs(curve, P):
    c = br.CURVES[curve]
    if P is None:
        return np.zeros((2, c.base.n_limbs), dtype=np.uint64), 1
    return np.array([c.base.mont_limbs(P[0]), c.base.mont_limbs(P[1])], dtype=np.uint64), 0


def expect(curve, pts):
    """points on integers -> (limbs (n, 2, L), zero flags): the unique affine form, (0, 0) and the flag for the identity"""
    rows = [point_limbs(curve, P) for P in pts]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], dtype=np.uint8)


_CACHE = {}


def ec_mul_cached(curve, k, P):
    key = (curve, k, P)
    if key not in _CACHE:
        _CACHE[key] = None if P is None else br.ec_mul(br.CURVES[curve], k, P)
    return _CACHE[key]


def check(curve, prs, out, oz):
    exp, ez = expect(curve, [ec_mul_cached(curve, k, P) for k, P in prs])
    bad = [i for i in range(len(prs)) if ez[i] != oz[i] or not np.array_equal(exp[i], out[i])]
    assert not bad, (curve, bad[:8], [hex(prs[i][0]) for i in bad[:8]])


# ---- the split along the endomorphism, restated on integers from glv.cuh; the lattice constants are read from glv_params.cuh as data ----
import functools
import os
import re

_GLV_NAMES = {0: "Tweedledee", 1: "Tweedledum", 3: "Pallas", 4: "Vesta"}
_GLV_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plonky_amd", "csrc", "glv_params.cuh")
GLV_BITS = 130
GLV_SHIFT = 384


@functools.lru_cache(maxsize=None)
def glv_params(curve):
    block = open(_GLV_FILE).read().split("struct %sGlv" % _GLV_NAMES[curve])[1].split("\n};")[0]

    def arr(name):
        ws = re.search(name + r"\[\d+\] = \{([^}]*)\}", block).group(1).split(",")
        return sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(ws))

    sign = lambda name: -1 if re.search(name + r"_NEG = (\w+)", block).group(1) == "true" else 1
    return {n: arr(n) * (sign(n) if n in ("A1", "B1", "A2", "B2") else 1) for n in ("LAMBDA", "G1", "G2", "A1", "B1", "A2", "B2")}


def glv_split(curve, k):
    """glv.cuh: m_i = floor(k G_i / 2^384), k1 = k - (m1 a1 + m2 a2), k2 = -(m1 b1 + m2 b2), as signed integers"""
    g = glv_params(curve)
    m1, m2 = (k * g["G1"]) >> GLV_SHIFT, (k * g["G2"]) >> GLV_SHIFT
    return k - (m1 * g["A1"] + m2 * g["A2"]), -(m1 * g["B1"] + m2 * g["B2"])


_SPLIT_CASES = {}


def glv_edge_scalars(curve):
    """Scalars chosen with the restated split: one half 0 and the other as long as that leaves it (the largest K that splits into
    (K, 0) and the largest that K lambda splits into (0, +-K), by bisection), and the scalars with the longest halves the search
    below finds - just under the values at which a quotient m_i steps, and the longest of 4000 seeded ones.  -> (scalars, longest half in bits)"""
    if curve in _SPLIT_CASES:
        return _SPLIT_CASES[curve]
    r = br.CURVES[curve].scalar.p
    g = glv_params(curve)
    lam = g["LAMBDA"]
    lo, hi = 0, 1 << GLV_BITS                         # split(K) == (K, 0) exactly while both quotients are 0: monotone in K
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if glv_split(curve, mid) == (mid, 0) else (lo, mid)
    out = [lo]
    assert glv_split(curve, lo) == (lo, 0) and glv_split(curve, lo + 1) != (lo + 1, 0) and lo.bit_length() >= 126
    # (0, K): the split returns the representative inside the cell spanned by the two basis vectors (its quotients are floors), and on
    # all four curves that cell does not hold the axis k1 = 0: no scalar but 0 splits into (0, k2).  Where a ray of it is inside, K runs
    # along it until it leaves the cell (monotone again); K lambda and -K lambda for K = 2^127 - 1 are cases either way.
    K = (1 << 127) - 1
    out += [K * lam % r, (r - K * lam) % r]
    for sg in (1, -1):
        if glv_split(curve, sg * lam % r) != (0, sg):
            continue
        lo2, hi2 = 1, 1 << GLV_BITS
        while hi2 - lo2 > 1:
            mid = (lo2 + hi2) // 2
            lo2, hi2 = (mid, hi2) if glv_split(curve, sg * mid * lam % r) == (0, sg * mid) else (lo2, mid)
        out.append(sg * lo2 * lam % r)
    cands = [((t << GLV_SHIFT) + g[n] - 1) // g[n] - 1 for n in ("G1", "G2") for t in (1, 2, 3, 5)]   # the last k before m_i reaches t
    cands += random_scalars(curve, 4242 + curve, 4000)
    cands = [k for k in cands if 0 <= k < r]
    halves = {k: glv_split(curve, k) for k in cands}
    for k, (k1, k2) in halves.items():
        assert (k1 + k2 * lam - k) % r == 0 and abs(k1) < (1 << GLV_BITS) and abs(k2) < (1 << GLV_BITS)
    out += sorted(cands, key=lambda k: -abs(halves[k][0]))[:2] + sorted(cands, key=lambda k: -abs(halves[k][1]))[:2]
    longest = max(max(abs(a), abs(b)) for a, b in (glv_split(curve, k) for k in out)).bit_length()
    _SPLIT_CASES[curve] = (out, longest)
    return _SPLIT_CASES[curve]


def power_pairs(curve):
    """(2^k, G) and (2^k - 1, G) for EVERY k below the scalar field's bit length: every bit, digit, word and limb boundary.  The
    expectations come from one chain of doublings ([2^k - 1] G = [2^k] G - G) and are put into the cache check() reads."""
    c = br.CURVES[curve]
    G = (c.gx, c.gy)
    neg_g = br.ec_neg(c, G)
    out, acc = [], G
    for k in range(1, c.scalar.bits):
        acc = br.ec_add(c, acc, acc)
        for s, P in (((1 << k) % c.scalar.p, acc), (((1 << k) - 1) % c.scalar.p, br.ec_add(c, acc, neg_g))):
            if (1 << k) < c.scalar.p:
                _CACHE[(curve, s, G)] = P
                out.append((s, G))
    return out
