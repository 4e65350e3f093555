"""Inputs and refusals of the gate-trace entries (include/plonky_hip_trace.h) as data, shared by the CPU tests (the restatement, the
host replay, the ABI) and the GPU test.  A plain helper module: no fixtures, no pytest settings."""
import ctypes

import numpy as np

from oracle import bigint_ref as br
from tests import gate_trace_ref as gt

ENTRIES = ("plk_trace_rescue_permutation_dev", "plk_trace_rescue_permutation", "plk_trace_curve_msm_dev", "plk_trace_curve_msm")
RESCUE_FIELDS = (0, 1, 4, 5)  # the 4-limb fields whose Rescue exponent is 5: Bls12377Scalar has 11, Bls12377Base six limbs
MSM_CURVES = (0, 1, 3, 4)     # the curves whose base field has 4 limbs: the wires are elements of it


def values(f, seed, count):
    return [f.from_mont(br.limbs_to_int(l)) for l in br.rand_field_limbs(f, seed, count)]


def points(curve, seed, count):
    """count distinct multiples of the generator: a seeded start, then steps of a seeded difference (affine adds on integers)"""
    c = br.CURVES[curve]
    g = (c.gx, c.gy)
    pt, step = br.ec_mul(c, 0x1000 + seed, g), br.ec_mul(c, 0x77 + 2 * seed, g)
    out = []
    for _ in range(count):
        out.append(pt)
        pt = br.ec_add(c, pt, step)
    return out


def start_point(curve):
    """the starting accumulator: any point serves as the builder's `filler`"""
    c = br.CURVES[curve]
    return br.ec_mul(c, 0xF111E4, (c.gx, c.gy))


def back_to_back(count, block, first=0):
    return [first + i * block for i in range(count)]


def scattered(count, block, seed):
    """blocks in a seeded order with seeded gaps of 0 .. 3 rows; returns (first_rows, rows needed)"""
    rng = np.random.default_rng(seed)
    order, gaps = rng.permutation(count), rng.integers(0, 4, count)
    first, at = [0] * count, 0
    for c, g in zip(order, gaps):
        at += int(g)
        first[int(c)] = at
        at += block
    return first, at


def msm_sum(curve, pts, scs):
    c = br.CURVES[curve]
    acc = None
    for p, s in zip(pts, scs):
        acc = br.ec_add(c, acc, br.ec_mul(c, s, p))
    return acc


def msm_result(curve, wires, first, parts, n_bits, start):
    """the block's result with the start multiple taken off: wires 0/1 of the last doubling row minus 2^(n_bits - 1) start"""
    c = br.CURVES[curve]
    last = first + gt.msm_block_rows(parts, n_bits) - 1
    return br.ec_add(c, (wires[(0, last)], wires[(1, last)]), br.ec_neg(c, br.ec_mul(c, 1 << (n_bits - 1), start)))


def x_collision_point(curve, pts, scs, start, n_bits, j_hit, i_hit):
    """An addend for part j_hit such that x1 = x2 first occurs at the add row of bit i_hit, part j_hit: the accumulator that row sees,
    computed on integers with the other parts as they are.  Returns the point (the accumulator itself)."""
    c = br.CURVES[curve]
    assert scs[j_hit] >> (i_hit + 1) == 0, "the part's own addend must not have gone into the accumulator before that row"
    acc = start
    for i in range(n_bits - 1, -1, -1):
        for j in range(len(pts)):
            if (i, j) == (i_hit, j_hit):
                return acc
            if (scs[j] >> i) & 1:
                acc = br.ec_add(c, acc, pts[j])
        acc = br.ec_add(c, acc, acc)
    raise AssertionError("no such row")


# ---- the refusals: (case name, overrides of the good call, the text plk_last_error starts with), in the documented order ----
MSM_ORDER = ("count", "parts", "n_bits", "curve", "points", "scalars", "start_xy", "n_rows", "wires", "first_rows", "constants", "status")
MSM_GOOD = dict(count=1, parts=2, n_bits=8, curve=0, points="p", scalars="p", start_xy="p", n_rows=64, wires="p", first_rows="p", constants="p", status="p")
MSM_REFUSALS = [
    ("unknown curve -1", dict(curve=-1), "bad curve id -1"),
    ("unknown curve 5", dict(curve=5), "bad curve id 5"),
    ("six-limb base field", dict(curve=2), "curve 2 has a 6-limb base field"),
    ("count 2^32", dict(count=1 << 32), "count 4294967296"),
    ("parts 0", dict(parts=0), "parts 0"),
    ("parts 9", dict(parts=9), "parts 9"),
    ("n_bits 0", dict(n_bits=0), "n_bits 0"),
    ("n_bits 255", dict(n_bits=255), "n_bits 255"),
    ("n_rows 0", dict(n_rows=0), "n_rows 0"),
    ("n_rows 2^27 + 1", dict(n_rows=(1 << 27) + 1), "n_rows 134217729"),
    ("null start_xy", dict(start_xy=None), "null pointer: start_xy"),
    ("null points", dict(points=None), "null pointer: points"),
    ("null scalars", dict(scalars=None), "null pointer: scalars"),
    ("null wires", dict(wires=None), "null pointer: wires"),
    ("null first_rows", dict(first_rows=None), "null pointer: first_rows"),
    # the order of the checks
    ("unknown curve and everything else wrong", dict(curve=9, count=1 << 32, parts=0, n_bits=0, n_rows=0, start_xy=None), "bad curve id 9"),
    ("six limbs before the count", dict(curve=2, count=1 << 32, parts=0), "curve 2 has a 6-limb base field"),
    ("count before parts", dict(count=1 << 32, parts=0, n_bits=0), "count 4294967296"),
    ("parts before n_bits", dict(parts=0, n_bits=0, n_rows=0), "parts 0"),
    ("n_bits before n_rows", dict(n_bits=300, n_rows=0, start_xy=None), "n_bits 300"),
    ("n_rows before start_xy", dict(n_rows=0, start_xy=None, points=None), "n_rows 0"),
    ("start_xy before the tables", dict(start_xy=None, points=None, scalars=None, wires=None, first_rows=None), "null pointer: start_xy"),
    ("everything else null", dict(points=None, scalars=None, wires=None, first_rows=None, constants=None, status=None), "null pointer: points"),
    ("scalars before wires", dict(scalars=None, wires=None, first_rows=None), "null pointer: scalars"),
    ("wires before first_rows", dict(wires=None, first_rows=None), "null pointer: wires"),
]
# with a context (a GPU is needed to make one): overrides over RESCUE_GOOD, `ctx` filled in by the caller
RESCUE_ORDER = ("count", "ctx", "inputs", "n_rows", "wires", "first_rows", "constants", "status")
RESCUE_GOOD = dict(count=1, ctx="ctx", inputs="p", n_rows=64, wires="p", first_rows="p", constants="p", status="p")
RESCUE_REFUSALS = [
    ("null context", dict(ctx=None), "null context"),
    ("null context before the count", dict(ctx=None, count=1 << 32, n_rows=0, inputs=None), "null context"),
    ("count 2^32", dict(count=1 << 32), "count 4294967296"),
    ("count before n_rows", dict(count=1 << 32, n_rows=0), "count 4294967296"),
    ("n_rows 0", dict(n_rows=0), "n_rows 0"),
    ("n_rows 2^27 + 1", dict(n_rows=(1 << 27) + 1), "n_rows 134217729"),
    ("n_rows before the pointers", dict(n_rows=0, inputs=None, wires=None, first_rows=None), "n_rows 0"),
    ("null inputs", dict(inputs=None), "null pointer: inputs"),
    ("null wires", dict(wires=None), "null pointer: wires"),
    ("null first_rows", dict(first_rows=None), "null pointer: first_rows"),
    ("everything null", dict(inputs=None, wires=None, first_rows=None, constants=None, status=None), "null pointer: inputs"),
    ("wires before first_rows", dict(wires=None, first_rows=None), "null pointer: wires"),
]


def refusal_results(L, entries, order, good, refusals, ctx=None):
    """[(entry, case name, code, text)] of every refusal through the given entries of the loaded library L; the pointers of the good
    call all name one small host buffer that no refused call reads"""
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    out = []
    for entry in entries:
        for name, override, _ in refusals:
            args = [dict(good, **override)[k] for k in order]
            args = [p if a == "p" else ctx if a == "ctx" else a for a in args]
            if entry.endswith("_dev"):
                args.append(None)  # the stream
            rc = getattr(L, entry)(*args)
            out.append((entry, name, int(rc), L.plk_last_error().decode()))
    return out
