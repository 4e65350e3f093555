"""Degenerate inputs of the inner-product argument (plk_halo_*, src/halo.rs:63-124) with a closed form.

Every point of a case is a known multiple of the curve's generator: halo_g[i] = [k_i] G (a flagged generator counts as k_i = 0),
H = [k_H] G, U' = [k_U] G.  A whole argument is then arithmetic modulo r on Python integers; with m = n / 2, per round
    L  = [ sum_{i<m} a_i k_{m+i} + l k_H + (sum_{i<m} a_i b_{m+i}) k_U ] G
    R  = [ sum_{i<m} a_{m+i} k_i + r k_H + (sum_{i<m} a_{m+i} b_i) k_U ] G
    a'_i = u^-1 a_{m+i} + u a_i,   b'_i = u^-1 b_i + u b_{m+i},   k'_i = u^-1 k_i + u k_{m+i}
and a point is the identity (flag 1, all-zero words) exactly when its logarithm is 0 mod r.  The challenges and the blinding factors
are inputs, so a case can choose its logarithms backwards from them.

A case names the branch it is built to reach and PLANS the positions at which an L / R or a fold output is the identity;
`identities` finds those positions from the integers alone and `build_cases` asserts that they are the planned ones - nothing is
left to chance.  tests/test_halo_degenerate_cases.py holds the table against the oracle; tests/test_gpu_halo_degenerate.py runs it
through every regime of the device context.  No GPU and no torch here."""
import random
from dataclasses import dataclass, field

import numpy as np

from oracle import bigint_ref as br

K_P = 0xC0FFEE          # the point of the "one point" family
X_INSIDE = 0x1234567 * 0x9E3779B97F4A7C15F39CC0605CEDC835   # U' = [x] U when H and U sit in the caller's tables

FAMILIES = ("flagged", "one_point", "opposite_halves", "fold_identities", "zero_scalars", "special_challenges", "hu_colliding")

# (family, regime, reason) for every family that cannot exist in a regime of tests/test_gpu_halo_degenerate.py: none - every family is
# a choice of logarithms, scalars and challenges, which every regime accepts (the CPU test asserts this list)
EXCEPTIONS = []


@dataclass
class Case:
    name: str
    family: str
    branch: str            # the exceptional branch the case reaches by construction
    c: object              # br.CurveSpec
    n: int
    k: list                # logarithms of halo_g (0 where flagged)
    flags: list            # identity flags of halo_g
    decoy: dict            # flagged index -> logarithm of the coordinates it carries (a valid point that must be ignored); absent: zeros
    a: list
    b: list
    k_h: int
    k_u: int
    blind: list            # (l_j, r_j) per round
    us: list               # u_j per round
    planned: set = field(default_factory=set)   # ("L", j) / ("R", j) / ("g", j, i): identities, j = round, i = position after its fold


@dataclass
class Round:
    L: int
    R: int
    a: list
    b: list
    k: list


def fold(p, u, a, b, k):
    m, ui = len(a) // 2, pow(u, -1, p)
    return ([(ui * a[m + i] + u * a[i]) % p for i in range(m)], [(ui * b[i] + u * b[m + i]) % p for i in range(m)],
            [(ui * k[i] + u * k[m + i]) % p for i in range(m)])


def lr_logs(p, a, b, k, k_h, k_u, l, r):
    m = len(a) // 2
    ip_l = sum(a[i] * b[m + i] for i in range(m))
    ip_r = sum(a[m + i] * b[i] for i in range(m))
    return ((sum(a[i] * k[m + i] for i in range(m)) + l * k_h + ip_l * k_u) % p,
            (sum(a[m + i] * k[i] for i in range(m)) + r * k_h + ip_r * k_u) % p)


def closed_form(case):
    """the logarithms of every L_j / R_j and the state after every fold"""
    p = case.c.scalar.p
    a, b, k = list(case.a), list(case.b), list(case.k)
    out = []
    for (l, r), u in zip(case.blind, case.us):
        L, R = lr_logs(p, a, b, k, case.k_h, case.k_u, l, r)
        a, b, k = fold(p, u, a, b, k)
        out.append(Round(L, R, a, b, k))
    return out


def identities(case):
    found = set()
    for j, rd in enumerate(closed_form(case)):
        found |= {(q, j) for q, v in (("L", rd.L), ("R", rd.R)) if v == 0}
        found |= {("g", j, i) for i, v in enumerate(rd.k) if v == 0}
    return found


# ---- points by their logarithm: [k] G from the table of [2^i] G, Jacobian with one inversion, cached ----
_POW2, _POINTS = {}, {}


def point(c, k):
    """[k mod r] G as affine integers, None for the identity"""
    k %= c.scalar.p
    if k == 0:
        return None
    key = (c.curve_id, k)
    if key in _POINTS:
        return _POINTS[key]
    if c.curve_id not in _POW2:
        tab = [(c.gx, c.gy)]
        for _ in range(c.scalar.p.bit_length() - 1):
            tab.append(br.ec_add(c, tab[-1], tab[-1]))
        _POW2[c.curve_id] = tab
    q = c.base.p
    X = Y = Z = None
    # the partial sum over the bits below i is a multiple smaller than 2^i: never +-[2^i] G, the mixed addition has no exception
    for i, (x2, y2) in enumerate(_POW2[c.curve_id]):
        if not (k >> i) & 1:
            continue
        if X is None:
            X, Y, Z = x2, y2, 1
            continue
        zz = Z * Z % q
        h, rr = (x2 * zz - X) % q, 2 * (y2 * Z * zz - Y) % q
        assert h
        hh = h * h % q
        ii = 4 * hh % q
        jj, v = h * ii % q, X * ii % q
        X3 = (rr * rr - jj - 2 * v) % q
        Y, Z = (rr * (v - X3) - 2 * Y * jj) % q, ((Z + h) * (Z + h) - zz - hh) % q
        X = X3
    zi = pow(Z, -1, q)
    P = (X * zi * zi % q, Y * zi * zi * zi % q)
    _POINTS[key] = P
    return P


def point_words(c, k):
    """((2, L) Montgomery limbs, flag) of [k] G as the library returns it: the identity is flag 1 with all-zero words"""
    P = point(c, k)
    if P is None:
        return np.zeros((2, c.base.n_limbs), dtype=np.uint64), 1
    return np.array([c.base.mont_limbs(P[0]), c.base.mont_limbs(P[1])], dtype=np.uint64), 0


def scalar_words(c, vals):
    f = c.scalar
    return np.array([f.mont_limbs(v) for v in vals], dtype=np.uint64).reshape(len(vals), f.n_limbs)


def case_arrays(case):
    """the inputs as the library and the oracle take them: g (n, 2, L), flags (n,), h, u' (2, L), a, b (n, 4), us (rounds, 4),
    blind (2 rounds, 4) - a flagged generator carries its decoy's coordinates, or zeros"""
    c = case.c
    g = np.stack([point_words(c, case.decoy.get(i, 0) if case.flags[i] else case.k[i])[0] for i in range(case.n)])
    gz = np.array(case.flags, dtype=np.uint8)
    blind = [v for lr in case.blind for v in lr]
    return (g, gz, point_words(c, case.k_h)[0], point_words(c, case.k_u)[0], scalar_words(c, case.a), scalar_words(c, case.b),
            scalar_words(c, case.us), scalar_words(c, blind))


def inside_u(case):
    """H and U inside the caller's tables: U = [k_u] G with k_u = k_U / x, u_prime_scalar = x -> ((2, L) words of U, x)"""
    p = case.c.scalar.p
    x = X_INSIDE % p
    return point_words(case.c, case.k_u * pow(x, -1, p))[0], x


# ---- special field elements ----
def sqrt_minus_one(p):
    """z^((r-1)/4) for the smallest non-residue z: all five scalar fields have r = 1 mod 4"""
    assert p % 4 == 1
    z = next(z for z in range(2, 100) if pow(z, (p - 1) // 2, p) == p - 1)
    s = pow(z, (p - 1) // 4, p)
    assert s * s % p == p - 1
    return s


def cube_root_of_unity(p):
    assert p % 3 == 1
    w = next(w for w in (pow(z, (p - 1) // 3, p) for z in range(2, 100)) if w != 1)
    assert pow(w, 3, p) == 1
    return w


# ---- the families ----
def _rng(c, n, tag):
    return random.Random("%s/%d/%s" % (c.name, n, tag))


def _generic(c, n, tag):
    """ordinary inputs: non-zero logarithms, scalars, blinding factors and challenges - what a family does not choose"""
    rng, p, rounds = _rng(c, n, tag), c.scalar.p, n.bit_length() - 1
    nz = lambda: rng.randrange(1, p)
    return dict(k=[nz() for _ in range(n)], flags=[0] * n, decoy={}, a=[nz() for _ in range(n)], b=[nz() for _ in range(n)], k_h=nz(), k_u=nz(),
                blind=[(nz(), nz()) for _ in range(rounds)], us=[rng.randrange(2, p - 1) for _ in range(rounds)])


def _case(c, n, family, name, branch, planned=(), **over):
    d = _generic(c, n, name)
    d.update(over)
    return Case(name=name, family=family, branch=branch, c=c, n=n, planned=set(planned), **d)


def _flagged(c, n):
    m, p = n // 2, c.scalar.p
    sets = [("lo_edges", [0, m - 1], "flags at 0 and m - 1: identities in R's MSM and on the lo side of a fold"),
            ("hi_edges", [m, n - 1], "flags at m and n - 1: identities in L's MSM (bound through gz + m) and on the hi side of a fold"),
            ("pair", [1, m + 1], "both members of pair 1 flagged: the fold's output is an identity that the next round reads"),
            ("quarter", list(range(m + m // 2, n)), "the whole top quarter flagged: a run of identities in the rebind, the tables and the fold"),
            ("corners", [0, m - 1, m, n - 1], "flags at 0, m - 1, m, n - 1: two all-identity pairs beside live ones")]
    out = []
    for tag, idx, branch in sets:
        d = _generic(c, n, "flagged_" + tag)
        for t, i in enumerate(idx):
            d["flags"][i] = 1
            if t % 2:   # every other flagged entry carries a valid point that only the flag cancels
                d["decoy"][i] = d["k"][i]
            d["k"][i] = 0
        planned = {("g", 0, i) for i in range(m) if i in idx and m + i in idx}
        out.append(Case(name="flagged_" + tag, family="flagged", branch=branch, c=c, n=n, planned=planned, **d))
    return out


def _one_point(c, n):
    return [_case(c, n, "one_point", "one_point", "every generator is P: every pair of every round is P == Q, every MSM runs over one point", k=[K_P] * n)]


def _opposite(c, n):
    m, p = n // 2, c.scalar.p
    d = _generic(c, n, "opposite_first")
    k = d["k"][:m] + [p - v for v in d["k"][:m]]
    a = d["a"][:m] * 2
    return [_case(c, n, "opposite_halves", "opposite_first", "g_hi = -g_lo in the first round, distinct points: Q == -P operands of the MSMs' sums", k=k),
            _case(c, n, "opposite_halves", "opposite_every_round",
                  "g_i = (-1)^popcount(i) P and a_lo = a_hi: g_hi = -g_lo in every round, L = -R up to the H and U' terms",
                  k=[K_P if bin(i).count("1") % 2 == 0 else p - K_P for i in range(n)], a=a)]


def _fold_identities(c, n):
    m, p, rounds = n // 2, c.scalar.p, n.bit_length() - 1
    every = {("g", j, i) for j in range(rounds) for i in range(n >> (j + 1))}
    out = []
    # (a) every pair of round 0 cancels: k_{m+i} = -u_0^-2 k_i
    d = _generic(c, n, "fold_all")
    w = p - pow(d["us"][0], -2, p)
    out.append(_case(c, n, "fold_identities", "fold_all", "every pair of round 0 folds to the identity: all later MSMs, the freeze and the final halo_g run over identities",
                     planned=every, k=d["k"][:m] + [w * v % p for v in d["k"][:m]]))
    # (b) a few pairs of round 0: 0, m - 1 and m / 2 - positions 0 and m / 2 then meet in round 1 as identity + identity
    d = _generic(c, n, "fold_some_round0")
    w = p - pow(d["us"][0], -2, p)
    k = list(d["k"])
    for i in (0, m - 1, m // 2):
        k[m + i] = w * k[i] % p
    out.append(_case(c, n, "fold_identities", "fold_some_round0", "pairs 0, m - 1, m / 2 of round 0 fold to the identity: identities beside live points when the next regime starts",
                     planned={("g", 0, 0), ("g", 0, m - 1), ("g", 0, m // 2), ("g", 1, 0)}, k=k))
    # (b') a few pairs of round 1: k^(1)_{m1+i} = -u_1^-2 k^(1)_i, solved for k_{m+m1+i}
    d = _generic(c, n, "fold_some_round1")
    u0, u0i, m1 = d["us"][0], pow(d["us"][0], -1, p), m // 2
    w = p - pow(d["us"][1], -2, p)
    k = list(d["k"])
    pos = [m1 - 1] + ([0] if m1 >= 4 else [])
    for i in pos:
        lo = (u0i * k[i] + u0 * k[m + i]) % p
        k[m + m1 + i] = (w * lo - u0i * k[m1 + i]) * u0i % p
    out.append(_case(c, n, "fold_identities", "fold_some_round1", "pairs of round 1 fold to the identity: a flag written by emit_affine after live rounds",
                     planned={("g", 1, i) for i in pos}, k=k))
    # (c) g_hi = g_lo and u^2 = -1
    d = _generic(c, n, "fold_equal_halves")
    out.append(_case(c, n, "fold_identities", "fold_equal_halves", "g_hi = g_lo with u^2 = -1: every pair of round 0 is P + [-1] P",
                     planned=every, k=d["k"][:m] * 2, us=[sqrt_minus_one(p)] + d["us"][1:]))
    return out


def _states(p, a, b, k, us):
    """(j, a, b, k) at the start of every round"""
    for j, u in enumerate(us):
        yield j, a, b, k
        a, b, k = fold(p, u, a, b, k)


def _zero_scalars(c, n):
    m, p, rounds = n // 2, c.scalar.p, n.bit_length() - 1
    fam = "zero_scalars"
    out = [_case(c, n, fam, "a_zero", "a = 0: MSMs whose only non-zero scalars are those of H and U', zero inner products", a=[0] * n),
           _case(c, n, fam, "a_lo_zero", "a_lo = 0: L's MSM has one non-zero scalar (H), its inner product is zero; R is ordinary", a=[0] * m + _generic(c, n, "a_lo_zero")["a"][m:]),
           _case(c, n, fam, "b_zero", "b = 0: zero inner products, U' takes a zero scalar in every round", b=[0] * n)]
    d = _generic(c, n, "all_zero")
    blind = [(0, 0) if j != 1 else lr for j, lr in enumerate(d["blind"])]
    out.append(_case(c, n, fam, "all_zero", "a = 0 and l = r = 0 (all rounds but round 1): L and R are the identity, lr_zero = (1, 1)",
                     planned={(q, j) for j in range(rounds) if j != 1 for q in "LR"}, a=[0] * n, blind=blind))
    # L (even rounds) or R (odd rounds) cancels as a sum of live terms: l = -(sum a_i k_{m+i} + ip k_U) / k_H
    d = _generic(c, n, "cancelled")
    blind = []
    for j, a, b, k in _states(p, d["a"], d["b"], d["k"], d["us"]):
        L, R = lr_logs(p, a, b, k, d["k_h"], d["k_u"], 0, 0)
        kh_inv = pow(d["k_h"], -1, p)
        l, r = d["blind"][j]
        blind.append(((p - L) * kh_inv % p, r) if j % 2 == 0 else (l, (p - R) * kh_inv % p))
    out.append(_case(c, n, fam, "cancelled", "L (even rounds) / R (odd rounds) is the identity as a sum of live terms, the other an ordinary point of the same call",
                     planned={("L" if j % 2 == 0 else "R", j) for j in range(rounds)}, blind=blind))
    return out


def _special_challenges(c, n):
    p, rounds = c.scalar.p, n.bit_length() - 1
    i, w = sqrt_minus_one(p), cube_root_of_unity(p)
    ring = [1, p - 1, i, w, p - i, w * w % p]
    out = []
    for tag, order in (("forward", ring), ("backward", [w, i, p - 1, 1, w * w % p, p - i])):
        us = [order[j % 6] for j in range(rounds)]
        out.append(_case(c, n, "special_challenges", "special_u_" + tag, "u = 1, r - 1, sqrt(-1), a cube root of unity, one per round, on ordinary generators: u^2 = 1, -1, lambda^2 in the fold's recoding",
                         us=us))
    return out


def _hu_colliding(c, n):
    m, p = n // 2, c.scalar.p
    fam = "hu_colliding"
    d = _generic(c, n, "h_equals_u")
    out = [_case(c, n, fam, "h_equals_u", "H == U': the last two generators of every MSM are one point", k_u=d["k_h"])]
    d = _generic(c, n, "u_minus_h")
    blind = []
    for j, a, b, k in _states(p, d["a"], d["b"], d["k"], d["us"]):
        mm = len(a) // 2
        blind.append((sum(a[i] * b[mm + i] for i in range(mm)) % p, sum(a[mm + i] * b[i] for i in range(mm)) % p))
    out.append(_case(c, n, fam, "u_minus_h", "U' = -H with l = <a_lo, b_hi>, r = <a_hi, b_lo>: the H and U' terms cancel each other inside the MSM",
                     k_u=p - d["k_h"], blind=blind))
    d = _generic(c, n, "h_in_upper_half")
    blind = [(d["a"][m - 1], d["blind"][0][1])] + d["blind"][1:]
    out.append(_case(c, n, fam, "h_in_upper_half", "H == g[n - 1] and l_0 = a[m - 1]: one point twice in L's MSM with one scalar", k_h=d["k"][n - 1], blind=blind))
    return out


_BUILDERS = (_flagged, _one_point, _opposite, _fold_identities, _zero_scalars, _special_challenges, _hu_colliding)
_CASES = {}


def build_cases(c, n):
    """every case of every family for n generators on curve c; the planned identity positions are the ones the integers give"""
    key = (c.curve_id, n)
    if key not in _CASES:
        cases = [case for build in _BUILDERS for case in build(c, n)]
        for case in cases:
            assert len(case.k) == len(case.a) == len(case.b) == len(case.flags) == n and len(case.us) == len(case.blind) == n.bit_length() - 1
            assert all((case.k[i] == 0) == bool(case.flags[i]) for i in range(n)) and case.k_h and case.k_u and all(case.us)
            assert all(case.flags[i] and v for i, v in case.decoy.items())
            found = identities(case)
            assert found == case.planned, (case.name, sorted(found ^ case.planned))
        _CASES[key] = cases
    return _CASES[key]
