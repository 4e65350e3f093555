"""GPU parity: MSMs whose bucket sums collide, against a closed form.

The geometry, ordering and knob suites draw their generators as G + m D, all distinct, with random scalars: the accumulation meets its
doubling branch once per window (one duplicated generator) and the reduction tail - row and column sums, tree levels, bit planes,
heavy-bucket chunks, k_msm_final - never meets an exceptional branch at all: a tail that mishandles "two partial sums are equal" or "a
partial sum is the identity in mid-chain" would pass them.  Here every generator is a known multiple k_i G of the curve's generator, so
that sum_i s_i G_i = [sum_i s_i k_i mod r] G: one ec_mul on Python integers, no oracle MSM, bit for bit (affine results are unique).

Families, and the branch each reaches by construction:
  * one point - every generator is P, the scalars are uniform below 2^w for the context's window w, with the edge scalars 0, 1 and r - 1
    in front: only the lowest window is populated (r - 1 apart) and bucket b holds count_b copies of one table entry, so every addition
    of the accumulation after a bucket's first finds P = Q (the doubling inside the mixed addition) or, later, m P + P.  In the tail the
    bucket sums are small multiples of one point: equal partial sums (the doubling inside xyzzz_add / xyzzz_add_q) are overwhelmingly
    likely at the row / column sums and tree levels - buckets with equal counts are everywhere - but no particular one is forced;
  * +-P, cancelling - generators alternate P, -P and the scalars are equal in pairs: every digit of a pair falls into the same bucket
    with opposite points, so EVERY bucket sum, every partial sum at every level of every tail and the result are the identity,
    deterministically: the "opposite points" branch of the accumulation and the identity-operand paths of every tail kernel, end to
    end.  The flag is 1 and the output all zero;
  * +-P with five pairs left unequal - the same, except that a handful of buckets per window survive: identities and live points mixed
    in every row, column and tree (an identity operand in mid-chain, on either side);
  * small multiples - generators k_i G with k_i cycling through +-1 .. +-8 and full-width scalars: a bucket holds a few entries of 16
    possible points per window, so equal and opposite operands are likely inside the buckets (not forced), and bucket sums are small
    multiples of one table entry, which makes collisions in the tail overwhelmingly likely (not forced);
  * one heavy bucket of equal points - every generator is P and every scalar the same full-width value v: each window's one bucket
    holds n copies of one table entry.  The heavy-bucket chunks have equal lengths, hence equal partial sums, and the tree over them
    doubles at every level (the last, shorter chunk apart), deterministically; every other bucket is the identity.  Result [n v] P.

Geometries: the smallest at which each path of the reduction exists (tests/test_gpu_msm_geometry.py, tests/test_gpu_msm_order.py); every
family runs twice on the same context (the second run reuses the workspaces).  The 2-torsion point of BLS12-377 is not used here: the
reference defines no MSM over it (tests/test_gpu_group_law.py presents it to the group law)."""
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import plonky_amd as pa
from oracle import bigint_ref as br
from tests.test_oracle_kats import mont_arr

KNOBS = ("PLK_MSM_SLICE", "PLK_MSM_GLOG")
K_P = 0xC0FFEE   # P = K_P G


@pytest.fixture(autouse=True)
def _restore_knobs():
    yield
    for k in KNOBS:
        os.environ.pop(k, None)


_POINTS = {}


def _bases(c, ks):
    """(n, 2, L) Montgomery limbs of k G for every k of ks (few distinct values)"""
    rows = {}
    for k in set(ks):
        if (c.curve_id, k) not in _POINTS:
            P = br.ec_mul(c, abs(k), (c.gx, c.gy))
            _POINTS[(c.curve_id, k)] = P if k > 0 else br.ec_neg(c, P)
        P = _POINTS[(c.curve_id, k)]
        rows[k] = np.array([c.base.mont_limbs(P[0]), c.base.mont_limbs(P[1])], dtype=np.uint64)
    return np.stack([rows[k] for k in ks])


# ---- generator sets: the multiples k_i ----
def ks_one_point(n):
    return [K_P] * n


def ks_plus_minus(n):
    return [K_P if i % 2 == 0 else -K_P for i in range(n)]


def ks_small_multiples(n):
    return [(1 + (i // 2) % 8) * (1 if i % 2 == 0 else -1) for i in range(n)]


# ---- scalar vectors: canonical integers ----
def s_one_point(c, n, w, seed):
    rng = random.Random(seed)
    s = [rng.randrange(1 << w) for _ in range(n)]
    s[:3] = [0, 1, c.scalar.p - 1]   # n >= 3 everywhere
    return s


def s_pairs(c, n, w, seed, unequal=0):
    rng = random.Random(seed)
    s = []
    for _ in range(n // 2):
        v = rng.randrange(c.scalar.p)
        s += [v, v]
    if n % 2:
        s.append(0)   # the generator without a partner does not take part
    for j in range(unequal):
        s[2 * (7 + 11 * j) + 1] = rng.randrange(c.scalar.p)
    return s


def s_full_width(c, n, w, seed):
    rng = random.Random(seed)
    return [rng.randrange(c.scalar.p) for _ in range(n)]


def s_heavy(c, n, w, seed):
    return [random.Random(seed).randrange(c.scalar.p >> 1, c.scalar.p)] * n


# (family, generator set, scalars)
FAMILIES = [
    ("one_point", ks_one_point, s_one_point),
    ("heavy_bucket", ks_one_point, s_heavy),
    ("cancelling", ks_plus_minus, s_pairs),
    ("cancelling_but_five", ks_plus_minus, lambda c, n, w, seed: s_pairs(c, n, w, seed, unequal=5)),
    ("small_multiples", ks_small_multiples, s_full_width),
]


def _expected(c, ks, s):
    return br.ec_mul(c, sum(a * b for a, b in zip(s, ks)) % c.scalar.p, (c.gx, c.gy))


def _ok(c, got, gz, exp):
    if exp is None:
        return gz == 1 and not np.asarray(got).any()
    want = np.array([c.base.mont_limbs(exp[0]), c.base.mont_limbs(exp[1])], dtype=np.uint64)
    return gz == 0 and np.array_equal(np.asarray(got).reshape(want.shape), want)


def _run_families(c, n, win, table_free, families, seed):
    contexts, failed = {}, []
    try:
        for name, ks_of, s_of in families:
            ks = ks_of(n)
            if ks_of not in contexts:
                contexts[ks_of] = pa.msm_precompute(c.curve_id, _bases(c, ks), 8, device_window=win, table_free=table_free)
            pre = contexts[ks_of]
            if win:
                assert pre.window == win
            s = s_of(c, n, pre.window, seed)
            exp = _expected(c, ks, s)
            if name == "cancelling":
                assert exp is None
            sm = mont_arr(c.scalar, s)
            for run in range(2):   # the second execution reuses the context's workspaces
                got, gz = pa.msm_execute_parallel(pre, sm)
                if not _ok(c, got, gz, exp):
                    failed.append((name, "run %d" % run, "flag %d" % gz))
    finally:
        for pre in contexts.values():
            pre.free()
    assert not failed, failed   # every family runs, so that a failure names all the families it shows in


FULL = (br.TWEEDLEDEE, br.BLS12_377, br.PALLAS)
EVERY = FULL + (br.TWEEDLEDUM, br.VESTA)
# (id, n, window, knobs, table-free, curves)
GEOMETRIES = [
    ("3000_w9_one_level", 3000, 9, {}, False, FULL),
    ("6000_w13_two_level", 6000, 13, {}, False, EVERY),
    ("6000_w13_slice2_head_pieces", 6000, 13, {"PLK_MSM_SLICE": "2"}, False, FULL),
    ("6000_w16_glog0", 6000, 16, {"PLK_MSM_GLOG": "0"}, False, FULL),
    ("6000_w16_glog3", 6000, 16, {"PLK_MSM_GLOG": "3"}, False, FULL),
    ("6000_w13_table_free", 6000, 13, {}, True, FULL),
    ("2p14+2_default_window", (1 << 14) + 2, 0, {}, False, EVERY),
    ("257_comb", 257, 0, {}, False, FULL),
]
CASES = [pytest.param(c, g, id="%s-%s" % (c.name, g[0])) for g in GEOMETRIES for c in g[5]]


@pytest.mark.parametrize("c,geometry", CASES)
def test_colliding_bucket_sums_match_the_closed_form(c, geometry):
    _, n, win, knobs, table_free, _ = geometry
    os.environ.update(knobs)   # read when a context is built
    _run_families(c, n, win, table_free, FAMILIES, 0xC011 + n + win)


@pytest.mark.parametrize("c", FULL, ids=lambda c: c.name)
def test_batch_of_one_point_and_cancelling(c):
    """two vectors in one call over the +-P generators at n = 6000, window 13: the "one point" scalars (here over P, -P: buckets of equal
    and opposite entries) and the cancelling pairs share one reduction; the second result is the identity"""
    n = 6000
    ks = ks_plus_minus(n)
    pre = pa.msm_precompute(c.curve_id, _bases(c, ks), 8, device_window=13)
    vecs = [s_one_point(c, n, pre.window, 0xBA7C), s_pairs(c, n, pre.window, 0xBA7D)]
    exps = [_expected(c, ks, s) for s in vecs]
    assert exps[0] is not None and exps[1] is None
    stack = np.stack([mont_arr(c.scalar, s) for s in vecs])
    failed = []
    for run in range(2):
        bxy, bz = pa.msm_execute_batch(pre, stack)
        failed += [("vector %d" % k, "run %d" % run) for k in range(2) if not _ok(c, bxy[k], int(bz[k]), exps[k])]
    pre.free()
    assert not failed, failed


def test_window20_one_point_and_heavy_bucket():
    """the 20-bit window over 2^16 + 37 generators (the tile-major ordering and the reduction a 2^20 MSM runs): every generator the same"""
    _run_families(br.TWEEDLEDEE, (1 << 16) + 37, 20, False, FAMILIES[:2], 0xC020)
