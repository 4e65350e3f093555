"""The case table of the plain XYZZ law's tests (tests/test_xyzz_cases.py checks the table on the host, tests/test_gpu_xyzz_law.py runs
it): inputs for the three kernels of curve_ops.hip that are built on ec.cuh - k_sum_affine, k_combine_partials, k_gen_bases - and the
results big integers give.

A point is NAMED by a pair (k, t): k G + t T with |k| <= 2^12 and, on BLS12-377 only, T = (p - 1, 0) the 2-torsion point of
tests/group_law_cases.py.  The name is the group element, so the expected value of a sum is one ec_mul on the sum of the names, whatever
the order in which a kernel adds.

k_sum_affine has a fixed schedule: lane t of 64 adds the points t, t + 64, ... with xyzz_madd, then block_sum folds lane t + d into lane t
with xyzz_add for d = 32 ... 1.  schedule() replays it on affine big-integer points and records, per operation, the site (madd, add@d), the
lane and the branch the law takes there - which depends on the group elements alone - next to the XYZZ representatives the kernel's
formulas give, so that "both operands have zz != 1 and differ" is a checked property of a case, not a hope.  Every builder below is aimed
at (site, branch, lane) triples that the host test finds in the replay.

A combine case is a hand-written set of exchange records (include/plonky_hip.h, plk_msm_partials_bytes) for k_combine_partials.

Everything is plain Python and deterministic; nothing here calls the library or the oracle."""
import functools
from collections import namedtuple

import numpy as np

from oracle import bigint_ref as br

LANES = 64
DS = (32, 16, 8, 4, 2, 1)
MAX_K = 1 << 12
FLAG = "flag"          # the identity: flag set; zero words in a sum list, 0xFF words in an exchange record
JUNK = "junk"          # words that are no curve point (all 0xFF): flagged in a sum list, NOT flagged in an exchange record
UNCHECKED = "unchecked"  # the expected value of a combine vector that reads a JUNK cell
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 193)
MADD_BRANCHES = ("left-identity", "generic", "double", "cancel")
ADD_BRANCHES = ("left-identity", "right-identity", "generic", "double", "cancel")
SITES = ("madd",) + tuple("add@%d" % d for d in DS)
PAIRS = tuple(("madd", b) for b in MADD_BRANCHES) + tuple(("add@%d" % d, b) for d in DS for b in ADD_BRANCHES)
T = (0, 1)

# site: a member of SITES; lane: the lane that runs the operation; a, b: the XYZZ representatives (None: identity) that meet there
# (b of a madd: the affine operand as (x, y, 1, 1))
Step = namedtuple("Step", "site branch lane a b")
# entries: names, FLAG or JUNK, one per slot of the list; aims: (site, branch, lane) triples the case was built for
SumCase = namedtuple("SumCase", "label curve_id entries aims")
# cells[r][s]: a name, FLAG or JUNK: slot s of rank r's record
CombineCase = namedtuple("CombineCase", "label curve_id world batch whole cells")


def P(k):
    return (k, 0)


def neg(name):
    return (-name[0], name[1])   # -T = T


def t_minus(k):
    return (-k, 1)


# ---------------------------------------------------------------------------------------------
# names -> big-integer points
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _multiples(curve_id):
    c = br.CURVES[curve_id]
    out = [None]
    for _ in range(MAX_K):
        out.append(br.ec_add(c, out[-1], (c.gx, c.gy)))
    return out


@functools.lru_cache(maxsize=None)
def point(curve_id, name):
    """the affine point of a name (canonical integers)"""
    c = br.CURVES[curve_id]
    k, t = name
    assert abs(k) <= MAX_K and t in (0, 1) and (k or t) and (not t or c is br.BLS12_377)
    Q = _multiples(curve_id)[abs(k)]
    if k < 0:
        Q = br.ec_neg(c, Q)
    return br.ec_add(c, Q, (c.base.p - 1, 0)) if t else Q


@functools.lru_cache(maxsize=None)
def _multiple(curve_id, k):
    c = br.CURVES[curve_id]
    return br.ec_mul(c, k, (c.gx, c.gy))


def named_sum(curve_id, names):
    """the sum of named points from the names alone: [sum k] G + [sum t mod 2] T (None: the identity)"""
    c = br.CURVES[curve_id]
    k, t = sum(n[0] for n in names), sum(n[1] for n in names) % 2
    Q = _multiple(curve_id, abs(k))
    if k < 0:
        Q = br.ec_neg(c, Q)
    return br.ec_add(c, Q, (c.base.p - 1, 0)) if t else Q


@functools.lru_cache(maxsize=None)
def _limbs(curve_id, name):
    c = br.CURVES[curve_id]
    x, y = point(curve_id, name)
    return np.array([c.base.mont_limbs(x), c.base.mont_limbs(y)], dtype=np.uint64)


def points_to_arrays(c, pts):
    """affine points (None: identity) -> ((n, 2, L) Montgomery limbs, (n,) zero flags)"""
    L = c.base.n_limbs
    xy, zero = np.zeros((len(pts), 2, L), dtype=np.uint64), np.zeros(len(pts), dtype=np.uint8)
    for i, Q in enumerate(pts):
        if Q is None:
            zero[i] = 1
        else:
            xy[i, 0], xy[i, 1] = c.base.mont_limbs(Q[0]), c.base.mont_limbs(Q[1])
    return xy, zero


# ---------------------------------------------------------------------------------------------
# the schedule of k_sum_affine, with the representatives of ec.cuh's formulas (a = 0)
# ---------------------------------------------------------------------------------------------
def _dbl_rep(p, a):
    x, y, zz, zzz = a
    u = 2 * y % p
    v = u * u % p
    w = u * v % p
    s = x * v % p
    m = 3 * x * x % p
    x3 = (m * m - 2 * s) % p
    r = (x3, (m * (s - x3) - w * y) % p, v * zz % p, w * zzz % p)
    return r if r[2] else None


def _add_rep(p, a, b, branch):
    if branch == "left-identity":
        return b
    if branch == "right-identity":
        return a
    if branch == "cancel":
        return None
    if branch == "double":
        return _dbl_rep(p, a)
    x1, y1, zz1, zzz1 = a
    x2, y2, zz2, zzz2 = b
    u1, u2, s1, s2 = x1 * zz2 % p, x2 * zz1 % p, y1 * zzz2 % p, y2 * zzz1 % p
    pp_, r = (u2 - u1) % p, (s2 - s1) % p
    pp = pp_ * pp_ % p
    ppp = pp_ * pp % p
    q = u1 * pp % p
    x3 = (r * r - ppp - 2 * q) % p
    return (x3, (r * (q - x3) - s1 * ppp) % p, zz1 * zz2 * pp % p, zzz1 * zzz2 * ppp % p)


def rep_to_affine(p, a):
    if a is None:
        return None
    x, y, zz, zzz = a
    i3 = pow(zzz, -1, p)
    iz = zz * i3 % p
    return (x * iz * iz % p, y * i3 % p)


def _branch(c, A, B, mixed):
    if A is None:
        return "left-identity"
    if B is None:
        assert not mixed
        return "right-identity"
    if A == B:
        return "double"
    if A == br.ec_neg(c, B):
        return "cancel"
    return "generic"


def schedule(curve_id, entries):
    """k_sum_affine on a list: (the affine sum or None, [Step ...] in lane order per site)"""
    c = br.CURVES[curve_id]
    p = c.base.p
    aff, rep, steps = [None] * LANES, [None] * LANES, []
    for t in range(LANES):
        for i in range(t, len(entries), LANES):
            if entries[i] in (FLAG, JUNK):
                continue
            B = point(curve_id, entries[i])
            b = (B[0], B[1], 1, 1)
            branch = _branch(c, aff[t], B, True)
            steps.append(Step("madd", branch, t, rep[t], b))
            # a mixed doubling is xyzz_mdbl of the affine operand: the doubling of the representative (x, y, 1, 1)
            rep[t] = _dbl_rep(p, b) if branch == "double" else _add_rep(p, rep[t], b, branch)
            aff[t] = br.ec_add(c, aff[t], B)
            assert rep_to_affine(p, rep[t]) == aff[t]
    for d in DS:
        for t in range(d):
            branch = _branch(c, aff[t], aff[t + d], False)
            steps.append(Step("add@%d" % d, branch, t, rep[t], rep[t + d]))
            rep[t] = _add_rep(p, rep[t], rep[t + d], branch)
            aff[t] = br.ec_add(c, aff[t], aff[t + d])
            assert rep_to_affine(p, rep[t]) == aff[t]
    return aff[0], steps


def sum_arrays(c, case):
    """the arrays plk_curve_sum_affine takes: ((k, 2, L) Montgomery limbs, (k,) zero flags)"""
    L, n = c.base.n_limbs, len(case.entries)
    xy, zero = np.zeros((n, 2, L), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    for i, e in enumerate(case.entries):
        if e == FLAG:
            zero[i] = 1
        elif e == JUNK:
            zero[i] = 1
            xy[i] = 0xFFFFFFFFFFFFFFFF
        else:
            xy[i] = _limbs(c.curve_id, e)
    return xy, zero


# ---------------------------------------------------------------------------------------------
# sum cases
# ---------------------------------------------------------------------------------------------
def _filler(i):
    return P(200 + 3 * i)   # distinct, positive, away from the small multiples the builders place


def _list(k, placed, fill_lanes=()):
    """k slots: `placed` {index: entry}, filler points in the slots of `fill_lanes`, flags elsewhere"""
    e = [_filler(i) if i % LANES in fill_lanes else FLAG for i in range(k)]
    for i, v in placed.items():
        e[i] = v
    return e


def _others(*lanes, modulus=LANES):
    """the lanes that do not reach any of `lanes` before the tree level of distance modulus / 2"""
    return tuple(u for u in range(LANES) if u % modulus not in lanes)


def build_madd_double(cid):
    return [SumCase("madd/double@%d" % t, cid, _list(t + 65, {t: P(5 + t), t + 64: P(5 + t)}, fill), (("madd", "double", t),))
            for t, fill in ((0, ()), (63, _others(63)))]


def build_madd_cancel(cid):
    return [SumCase("madd/cancel@%d" % t, cid, _list(t + 129, {t: P(7 + t), t + 64: P(-7 - t), t + 128: P(90)}, fill),
                    (("madd", "cancel", t), ("madd", "left-identity", t)))
            for t, fill in ((0, _others(0)), (63, ()))]


def build_flags(cid):
    out = [SumCase("madd/after-flag@%d" % t, cid, _list(t + 65, {t + 64: P(11 + t)}, fill), (("madd", "left-identity", t),))
           for t, fill in ((0, ()), (63, _others(63)))]
    out.append(SumCase("madd/after-junk", cid, _list(130, {0: JUNK, 1: JUNK, 64: P(13), 65: JUNK, 129: P(14), 63: JUNK, 127: JUNK}),
                       (("madd", "left-identity", 0), ("madd", "left-identity", 1))))
    out.append(SumCase("all-flagged", cid, [JUNK if i % 3 == 0 else FLAG for i in range(130)], ()))
    return out


def _tree_pair(cid, d, t, sign, fill):
    j = DS.index(d)
    a, b, c2, d2 = 3 + 20 * j, 10 + 20 * j, 6 + 20 * j, 7 + 20 * j     # a + b = c2 + d2, {a, b} != {c2, d2}
    placed = {t: P(a), t + 64: P(b), t + d: P(sign * c2), t + d + 64: P(sign * d2)}
    fill_lanes = _others(t, t + d, modulus=2 * d) if fill else ()
    return _list(128, placed, fill_lanes)


def _ends(d, fill_first):
    """the first and the last lane of the tree level of distance d, one of them among filler points"""
    return [(0, fill_first)] + ([(d - 1, not fill_first)] if d > 1 else [])


def build_tree_double(cid):
    return [SumCase("add@%d/double@%d" % (d, t), cid, _tree_pair(cid, d, t, 1, fill), (("add@%d" % d, "double", t),))
            for d in DS for t, fill in _ends(d, False)]


def build_tree_cancel(cid):
    return [SumCase("add@%d/cancel@%d" % (d, t), cid, _tree_pair(cid, d, t, -1, fill), (("add@%d" % d, "cancel", t),))
            for d in DS for t, fill in _ends(d, True)]


def build_tree_identities(cid):
    out = []
    for d in DS:
        # only the lanes d .. 2d - 1 hold points: lane t < d is empty when lane t + d arrives
        out.append(SumCase("add@%d/left-identity" % d, cid, [FLAG] * d + [P(30 + i) for i in range(d)],
                           tuple(("add@%d" % d, "left-identity", t) for t in (0, d - 1))))
        # k = d < 64: only the lanes below d hold points
        out.append(SumCase("add@%d/right-identity" % d, cid, [P(60 + i) for i in range(d)],
                           tuple(("add@%d" % d, "right-identity", t) for t in (0, d - 1))))
    return out


def build_sizes(cid):
    out = []
    for k in SIZES:
        e = [_filler(i) for i in range(k)]
        aims = []
        if k >= 1:
            aims.append(("madd", "left-identity", 0))
        if k == 64:
            aims += [("add@%d" % d, "generic", t) for d in DS for t in (0, d - 1)]
        if k > 64:
            e[64] = e[0]                      # the first lane doubles
            aims.append(("madd", "double", 0))
        if k >= 127:
            aims.append(("madd", "generic", 1))
        if k >= 128:
            e[127] = neg(e[63])               # the last lane cancels
            aims.append(("madd", "cancel", 63))
        if k >= 193:
            aims += [("madd", "left-identity", 63), ("madd", "generic", 0)]   # 191 lands on the emptied lane, 192 on the doubled one
        out.append(SumCase("size-%d" % k, cid, e, tuple(aims)))
    return out


def build_torsion(cid):
    if br.CURVES[cid] is not br.BLS12_377:
        return []
    out = [SumCase("T+T", cid, _list(65, {0: T, 64: T}), (("madd", "double", 0),)),
           SumCase("T+T+P", cid, _list(192, {63: T, 127: T, 191: P(9)}, _others(63)), (("madd", "double", 63), ("madd", "left-identity", 63)))]
    for d in (32, 1):
        placed = {0: P(21), 64: t_minus(21), d: P(34), d + 64: t_minus(34)}
        out.append(SumCase("add@%d/double-T" % d, cid, _list(128, placed), (("add@%d" % d, "double", 0),)))
    return out


BUILDERS = (build_madd_double, build_madd_cancel, build_flags, build_tree_double, build_tree_cancel, build_tree_identities, build_sizes,
            build_torsion)


@functools.lru_cache(maxsize=None)
def sum_cases(curve_id):
    out = [case for build in BUILDERS for case in build(curve_id)]
    assert len({case.label for case in out}) == len(out)
    return tuple(out)


# ---------------------------------------------------------------------------------------------
# combine cases
# ---------------------------------------------------------------------------------------------
WORLDS = (1, 2, 3, 4, 5, 7, 8, 64, 65, 130)
SMALL_CONTENTS = ("distinct", "checker", "one-flagged", "all-but-one", "all-flagged", "same-two", "same-all", "opposite", "opposite-third",
                  "junk-beside-whole")
BIG_CONTENTS = ("distinct", "collide-64", "all-flagged")


def geometries(world):
    """(name, batch, whole_per_rank) with slots >= 5: the flag byte sits at every position of its 32-bit word"""
    g = [("sharded", 5, 0), ("whole", 5 * world, 5), ("below-floor", 2 * world + 4, 1)]
    if world >= 2:
        g.append(("hybrid-1", 4 * world + 1, 4))
    if world >= 3:
        g.append(("hybrid-2", 3 * world + 2, 3))
    if world >= 4:
        whole = max(1, 6 - world)
        g.append(("hybrid-w-1", whole * world + world - 1, whole))
    return g


def slots_of(world, batch, whole):
    return whole + (batch - whole * world)


def _cell(r, s):
    return P(1 + r + 140 * (s % 29))   # distinct over the ranks of a slot


def _cells(content, world, slots, whole):
    cells = [[_cell(r, s) for s in range(slots)] for r in range(world)]
    last = world - 1
    for s in range(slots):
        col = lambda r, v: cells[r].__setitem__(s, v)
        if content == "checker":           # a set flag between clear ones and a clear flag between set ones, along the record
            for r in range(world):
                if (r + s) % 2:
                    col(r, FLAG)
        elif content == "one-flagged":
            col(s % world, FLAG)
        elif content == "all-but-one":
            for r in range(world):
                if r != s % world:
                    col(r, FLAG)
        elif content == "all-flagged":
            for r in range(world):
                col(r, FLAG)
        elif content == "same-two":
            col(last, cells[0][s])
        elif content == "same-all":
            for r in range(world):
                col(r, cells[0][s])
        elif content in ("opposite", "opposite-third"):
            keep = 3 if content == "opposite-third" else 2
            for r in range(keep, world):
                col(r, FLAG)
            if world >= 2:
                col(1, neg(cells[0][s]))
        elif content == "junk-beside-whole":
            if s < whole:                  # the slot of a whole vector: real on one rank, words that are no point on the others
                for r in range(world):
                    if r != s % world:
                        col(r, JUNK)
        elif content == "collide-64":      # ranks that share a lane of the stride loop (or, at world 64, the ends of the tree)
            far = 64 if world > 64 else last
            col(far, cells[0][s])          # lane 0 doubles
            if world > 65:
                col(65, neg(cells[1][s]))  # lane 1 cancels, and rank 129 lands on the emptied accumulator
        elif content == "T-two":
            for r in range(world):
                col(r, FLAG)
            col(0, T)
            col(last, T)
            if world >= 3:
                col(1, _cell(1, s))
        else:
            assert content == "distinct"
    return tuple(tuple(row) for row in cells)


@functools.lru_cache(maxsize=None)
def combine_cases(curve_id):
    out = []
    for world in WORLDS:
        contents = SMALL_CONTENTS if world <= 8 else BIG_CONTENTS
        if world <= 8 and br.CURVES[curve_id] is br.BLS12_377:
            contents = contents + ("T-two",)
        for gname, batch, whole in geometries(world):
            for content in contents:
                if world > 8 and content != "distinct" and gname not in ("sharded", "hybrid-1"):
                    continue
                slots = slots_of(world, batch, whole)
                out.append(CombineCase("w%d/%s/%s" % (world, gname, content), curve_id, world, batch, whole, _cells(content, world, slots, whole)))
    return tuple(out)


def record_bytes(c, slots):
    """plk_msm_partials_bytes, recomputed"""
    return (slots * 2 * c.base.n_limbs * 8 + slots + 15) & ~15


def vector_cells(case, v):
    """the cells vector v is made of: its owner's slot (a whole vector) or one slot of every rank (a sharded one)"""
    if v < case.whole * case.world:
        return [case.cells[v % case.world][v // case.world]]
    s = case.whole + (v - case.whole * case.world)
    return [case.cells[r][s] for r in range(case.world)]


def combine_layout(case):
    """(the `world` records back to back as bytes, the `batch` expected points: affine, None or UNCHECKED)"""
    c = br.CURVES[case.curve_id]
    slots = slots_of(case.world, case.batch, case.whole)
    assert all(len(row) == slots for row in case.cells) and len(case.cells) == case.world
    rec, pts = record_bytes(c, slots), slots * 2 * c.base.n_limbs * 8
    buf = np.full((case.world, rec), 0xFF, dtype=np.uint8)   # the padding, and the coordinates under a set flag, stay 0xFF
    for r, row in enumerate(case.cells):
        xy = buf[r, :pts].view(np.uint64).reshape(slots, 2, c.base.n_limbs)
        for s, e in enumerate(row):
            buf[r, pts + s] = 1 if e == FLAG else 0
            if e not in (FLAG, JUNK):
                xy[s] = _limbs(case.curve_id, e)
    expected = []
    for v in range(case.batch):
        cells = vector_cells(case, v)
        expected.append(UNCHECKED if JUNK in cells else named_sum(case.curve_id, [e for e in cells if e != FLAG]))
    return buf.reshape(-1), expected
