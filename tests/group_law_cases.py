"""The case table of the group-law tests (tests/test_group_law_cases.py checks the table on the host, tests/test_gpu_group_law.py runs it
through plk_curve_op): operands for the point arithmetic of ecz.cuh / ecz_coop.cuh and the result big integers give.

Every operand is a signed multiple k G of the curve's generator with |k| < 2^20, drawn from a pool of 64 multiples per curve (48 seeded
ones and the doubles of the first 16, so that "B = -2A" exists), or the identity (k = 0), and travels with a non-zero lambda: the kernel
works on the XYZZ representative (x l^2, y l^3, l^2, l^3), so equal points arrive with different coordinates.  Lambdas cycle through
1, 2, p - 1 and seeded values, and the two operands of an element never share one.  The expected result of an operation is one
bigint_ref.ec_add / ec_mul on the affine operands.  On BLS12-377 the table also holds the 2-torsion point T = (p - 1, 0)
(y^2 = x^3 + 1), which is no multiple of G: its cases are marked k = "T".

Everything is seeded and plain Python; nothing here calls the library or the oracle."""
import functools
import random
from collections import Counter, namedtuple

import numpy as np

from oracle import bigint_ref as br

OPS = {"add": 0, "dbl": 1, "add_q": 2, "dbl_q": 3, "madd": 4, "madd_entry": 5, "dbl_q_times": 6, "wave_sum_q": 7, "chain_q": 8}
ONE_LANE, QUAD = "one-lane", "quad"
LAW = {"add": ONE_LANE, "dbl": ONE_LANE, "madd": ONE_LANE, "madd_entry": ONE_LANE,
       "add_q": QUAD, "dbl_q": QUAD, "dbl_q_times": QUAD, "wave_sum_q": QUAD, "chain_q": QUAD}
INFLATE, NEGATE = 1, 2
LENGTHS = (1, 3, 63, 64, 65, 257)   # cut quads, waves (64 lanes = 16 quads) and blocks (256 threads = 64 quads)
MAX_ELEMENTS = 2048
TIMES = (1, 13, 20)
GROUPS = (1, 2, 4, 8, 16)
T = "T"

PAIR_CLASSES = ("ordinary", "equal", "opposite", "id_first", "id_second", "id_both")
MIXED_CLASSES = ("ordinary", "equal", "opposite", "id_first")          # the affine operand of a mixed addition is never the identity
CHAIN_CLASSES = ("ordinary", "equal", "opposite", "b_is_minus_2a", "id_first", "id_second", "id_both")
WAVE_CLASSES = ("equal", "alternating", "mixed", "identities", "double_then_cancel")
T_CLASSES = ("dbl_T", "T_plus_T", "T_plus_P", "P_plus_T")

# k: the signed multiple of G (0: the identity, T: the 2-torsion point), lam: the representative's lambda
Operand = namedtuple("Operand", "k lam")
# a, b: Operand (b None for the one-operand operations); flags: INFLATE | NEGATE; cls: the class the element was built for
Element = namedtuple("Element", "a b flags cls")
# op: a key of OPS; param: doublings (dbl_q_times) or quads per group (wave_sum_q); expected: one affine point (None: identity) per result
Call = namedtuple("Call", "op param elements expected")


class Pool:
    def __init__(self, c):
        self.c = c
        rng = random.Random(0x6C0 + c.curve_id)
        ks = rng.sample(range(3, 1 << 19), 48)
        ks += [2 * k for k in ks[:16]]
        G = (c.gx, c.gy)
        self.ks = ks
        self.points = {k: br.ec_mul(c, k, G) for k in ks}
        self.rng = rng
        self._lam = 0

    def point(self, k):
        if k == 0:
            return None
        if k == T:
            return (self.c.base.p - 1, 0)
        P = self.points[abs(k)]
        return P if k > 0 else br.ec_neg(self.c, P)

    def k(self):
        k = self.rng.choice(self.ks)
        return k if self.rng.random() < 0.5 else -k

    def lam(self, other=None):
        p = self.c.base.p
        while True:
            self._lam += 1
            v = (1, 2, p - 1)[self._lam % 5] if self._lam % 5 < 3 else self.rng.randrange(3, p - 1)
            if v != other:
                return v

    def pair(self, ka, kb):
        la = self.lam()
        return Operand(ka, la), Operand(kb, self.lam(other=la))


def _slices(elements, lengths):
    out, at = [], 0
    for n in lengths:
        out.append(elements[at:at + n])
        at += n
    assert at == len(elements)
    return out


def _pair_operands(pool, cls):
    ka = pool.k()
    if cls == "ordinary":
        kb = pool.k()
        while abs(kb) == abs(ka):
            kb = pool.k()
    else:
        kb = {"equal": ka, "opposite": -ka, "id_first": pool.k(), "id_second": 0, "id_both": 0, "b_is_minus_2a": None}[cls]
    if cls in ("id_first", "id_both"):
        ka = 0
    if cls == "b_is_minus_2a":
        ka = pool.rng.choice(pool.ks[:16]) * pool.rng.choice((1, -1))
        kb = -2 * ka
    return ka, kb


@functools.lru_cache(maxsize=None)
def calls(curve_id):
    """every call of the table for one curve, in a fixed order"""
    c = br.CURVES[curve_id]
    pool = Pool(c)
    add, dbl = (lambda P, Q: br.ec_add(c, P, Q)), (lambda P: br.ec_add(c, P, P))
    pt = pool.point
    total = sum(LENGTHS)
    out = []

    def emit(op, param, elements, expected):
        assert len(elements) <= MAX_ELEMENTS
        out.append(Call(op, param, tuple(elements), tuple(expected)))

    # additions of two XYZZ operands, one-lane and quad
    for op in ("add", "add_q"):
        els = []
        for i in range(total):
            cls = PAIR_CLASSES[i % len(PAIR_CLASSES)]
            a, b = pool.pair(*_pair_operands(pool, cls))
            els.append(Element(a, b, INFLATE if (i // len(PAIR_CLASSES)) % 2 else 0, cls))
        for part in _slices(els, LENGTHS):
            emit(op, 0, part, [add(pt(e.a.k), pt(e.b.k)) for e in part])
    # mixed additions: B is affine (its lambda is not read); madd_entry negates B when the flag says so
    for op in ("madd", "madd_entry"):
        els = []
        for i in range(total):
            cls = MIXED_CLASSES[i % len(MIXED_CLASSES)]
            ka, kb = _pair_operands(pool, cls)
            flags = INFLATE if (i // len(MIXED_CLASSES)) % 2 else 0
            if op == "madd_entry" and (i // (2 * len(MIXED_CLASSES))) % 2:
                flags, kb = flags | NEGATE, -kb   # the class describes A and the point that is added
            els.append(Element(Operand(ka, pool.lam()), Operand(kb, 1), flags, cls))
        for part in _slices(els, LENGTHS):
            emit(op, 0, part, [add(pt(e.a.k), pt(-e.b.k if e.flags & NEGATE else e.b.k)) for e in part])
    # doublings
    for op in ("dbl", "dbl_q"):
        els = []
        for i in range(total):
            cls = "identity" if i % 8 == 7 else "ordinary"
            els.append(Element(Operand(0 if cls == "identity" else pool.k(), pool.lam()), None, INFLATE if (i // 8) % 2 else 0, cls))
        for part in _slices(els, LENGTHS):
            emit(op, 0, part, [dbl(pt(e.a.k)) for e in part])
    # the planes doubled into place
    for times, lengths in zip(TIMES, ((3, 65), (1, 64), (63, 257))):
        els = []
        for i in range(sum(lengths)):
            ident = i % 16 == 15
            els.append(Element(Operand(0 if ident else pool.k(), pool.lam()), None, INFLATE if (i // 4) % 2 else 0, "times_%d" % times))
        for part in _slices(els, lengths):
            emit("dbl_q_times", times, part, [br.ec_mul(c, 1 << times, pt(e.a.k)) for e in part])
    # wave sums: 8 groups of every class per group size, and a short last group
    for q in GROUPS:
        els, exp = [], []
        classes = [w for w in WAVE_CLASSES if w != "double_then_cancel" or q >= 4]
        for g in range(8 * len(classes) + 1):
            cls = classes[g % len(classes)]
            last = g == 8 * len(classes)
            size = max(1, q // 2) if last else q
            k0 = pool.k()
            if cls == "equal":
                ks = [k0] * size
            elif cls == "alternating":
                ks = [k0 if j % 2 == 0 else -k0 for j in range(size)]
            elif cls == "double_then_cancel":
                ks = [k0 if j % 4 < 2 else -k0 for j in range(size)]
            elif cls == "identities":
                ks = [0 if pool.rng.random() < 0.4 or g % (2 * len(classes)) == classes.index(cls) else pool.k() for _ in range(size)]
            else:
                ks = [pool.k() for _ in range(size)]
            flags = INFLATE if (g // len(classes)) % 2 else 0
            els += [Element(Operand(k, pool.lam()), None, flags, "short_group" if last else cls) for k in ks]
            s = None
            for k in ks:
                s = add(s, pt(k))
            exp.append(s)
        emit("wave_sum_q", q, els, exp)
    # results of the quad law fed back into it: 2 (2A + B)
    els = []
    for i in range(total):
        cls = CHAIN_CLASSES[i % len(CHAIN_CLASSES)]
        a, b = pool.pair(*_pair_operands(pool, cls))
        els.append(Element(a, b, INFLATE if (i // len(CHAIN_CLASSES)) % 2 else 0, cls))
    for part in _slices(els, LENGTHS):
        emit("chain_q", 0, part, [dbl(add(add(pt(e.a.k), pt(e.b.k)), pt(e.a.k))) for e in part])
    # the 2-torsion point of BLS12-377
    if c is br.BLS12_377:
        for op in ("dbl", "dbl_q"):
            els = [Element(Operand(T, pool.lam()), None, INFLATE if i % 2 else 0, "dbl_T") for i in range(16)]
            emit(op, 0, els, [dbl(pt(T)) for _ in els])
        for op in ("add", "add_q", "madd", "madd_entry"):
            els = []
            for i in range(48):
                cls = T_CLASSES[1 + i % 3]
                ka, kb = {"T_plus_T": (T, T), "T_plus_P": (T, pool.k()), "P_plus_T": (pool.k(), T)}[cls]
                flags = INFLATE if (i // 3) % 2 else 0
                if op == "madd_entry" and (i // 6) % 2:
                    flags, kb = flags | NEGATE, (kb if kb == T else -kb)   # -T = T
                if op in ("madd", "madd_entry"):
                    els.append(Element(Operand(ka, pool.lam()), Operand(kb, 1), flags, cls))
                else:
                    els.append(Element(*pool.pair(ka, kb), flags, cls))
            neg = lambda e: e.b.k if e.b.k == T or not e.flags & NEGATE else -e.b.k
            emit(op, 0, els, [add(pt(e.a.k), pt(neg(e))) for e in els])
    return tuple(out)


def point(curve_id, k):
    """the affine point an Operand's k stands for (canonical integers; None: the identity)"""
    return _pool(curve_id).point(k)


@functools.lru_cache(maxsize=None)
def _pool(curve_id):
    return Pool(br.CURVES[curve_id])


def class_counts(curve_id):
    """(law, class, inflated) -> number of elements (wave sums: of groups)"""
    n = Counter()
    for call in calls(curve_id):
        if call.op == "wave_sum_q":
            for g in range(len(call.expected)):
                e = call.elements[g * call.param]
                n[(QUAD, "wave_" + e.cls, bool(e.flags & INFLATE))] += 1
        else:
            for e in call.elements:
                n[(LAW[call.op], e.cls, bool(e.flags & INFLATE))] += 1
    return n


def points_to_arrays(c, pts):
    """affine points (None: identity) -> ((n, 2, L) Montgomery limbs, (n,) zero flags)"""
    L = c.base.n_limbs
    xy, zero = np.zeros((len(pts), 2, L), dtype=np.uint64), np.zeros(len(pts), dtype=np.uint8)
    for i, P in enumerate(pts):
        if P is None:
            zero[i] = 1
        else:
            xy[i, 0], xy[i, 1] = c.base.mont_limbs(P[0]), c.base.mont_limbs(P[1])
    return xy, zero


def operand_arrays(c, call, which):
    """the arrays of operand `which` ("a" / "b") of a call: (points, zero flags, lambdas (n, L)), or None when the call has no such operand"""
    ops = [getattr(e, which) for e in call.elements]
    if ops[0] is None:
        return None
    xy, zero = points_to_arrays(c, [point(c.curve_id, o.k) for o in ops])
    lam = np.array([c.base.mont_limbs(o.lam) for o in ops], dtype=np.uint64).reshape(len(ops), c.base.n_limbs)
    return xy, zero, lam


def flag_array(call):
    return np.array([e.flags for e in call.elements], dtype=np.uint8)
