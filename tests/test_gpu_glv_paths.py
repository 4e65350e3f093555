"""The three device paths that run behind the endomorphism split (glv.cuh) on scalars chosen by what their HALVES look like
(tests/glv_half_cases.py; tests/test_glv_half_cases.py states what the pools hold): the table-free MSM, which recodes each half into
signed c-bit windows (ord_digit / ord_digit_at with raw_signed = 1), the pairwise generator fold (two joint sparse forms aligned at
the least significant column, k_fold_digits) and the 2^r-to-1 fold (one form per input, k_fold_multi_digits).  Every point is a known
multiple of the generator, so every expectation is one scalar multiplication on Python integers; comparisons are bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import plonky_amd as pa
from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from tests import glv_half_cases as gh
from tests.test_oracle_kats import from_mont_arr, mont_arr

CURVES = [br.CURVES[cv] for cv in gh.ENDO_CURVES]
_BASES = {}


def _pt(c, P):
    return np.array([c.base.mont_limbs(P[0]), c.base.mont_limbs(P[1])], dtype=np.uint64)


def _bases(c, n):
    """G_i = G + i D with D = [d] G -> ((n, 2, L) Montgomery limbs, the logarithms 1 + i d)"""
    if (c.curve_id, n) not in _BASES:
        G = (c.gx, c.gy)
        d = 0x9E3779B97F4A7C15 + c.curve_id
        pts = ol.gen_bases(c.curve_id, n, _pt(c, G), _pt(c, br.ec_mul(c, d, G)))
        _BASES[(c.curve_id, n)] = (pts, [(1 + i * d) % c.scalar.p for i in range(n)])
    pts, logs = _BASES[(c.curve_id, n)]
    return pts.copy(), list(logs)


def _multiple(c, k):
    """[k] G as (limbs (2, L), zero flag): the unique affine form, zeros and the flag for the identity"""
    k %= c.scalar.p
    if k == 0:
        return np.zeros((2, c.base.n_limbs), dtype=np.uint64), 1
    return _pt(c, br.ec_mul(c, k, (c.gx, c.gy))), 0


def _same(got, gz, exp, ez):
    return int(gz) == ez and np.array_equal(np.asarray(got), exp)


def _dot(ks, logs, flags=None):
    return sum(k * l for i, (k, l) in enumerate(zip(ks, logs)) if flags is None or not flags[i])


def _localise(c, pre, pool, logs, flags):
    """after a wrong sum: the pool again in halves (the other scalars set to 0) until one scalar is left - at most 7 executions"""
    idx = list(range(len(pool)))
    while len(idx) > 1:
        for part in (idx[:len(idx) // 2], idx[len(idx) // 2:]):
            ks = [pool[i].k if i in part else 0 for i in range(len(pool))]
            got, gz = pa.msm_execute_parallel(pre, mont_arr(c.scalar, ks))
            if not _same(got, gz, *_multiple(c, _dot(ks, logs, flags))):
                idx = part
                break
        else:
            return "both halves of %s are right on their own" % [pool[i].label for i in idx]
    m = pool[idx[0]]
    return "scalar %d '%s' k = %#x, halves (%#x, %#x)" % (idx[0], m.label, m.k, m.k1, m.k2)


@pytest.mark.parametrize("win", gh.WINDOWS)
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_table_free_msm_on_the_half_pool(c, win):
    """sum_i [k_i] G_i over the pool of window `win` = [sum_i k_i (1 + i d)] G: twice on one table-free context, with an identity flag and
    a repeated generator, as one vector of a batch beside all-zero and all-(r - 1), and through a tabled context of the same window
    (no split there: a difference says which side is wrong).  win = 13, 16 take the two-level reduction, 10 and 13 leave the top window empty."""
    r = c.scalar.p
    pool = gh.half_pool(c.curve_id, win)
    n = len(pool)
    ks = [m.k for m in pool]
    bases, logs = _bases(c, n)
    scalars = mont_arr(c.scalar, ks)
    exp, ez = _multiple(c, _dot(ks, logs))
    tabled = pa.msm_precompute(c.curve_id, bases, 8, device_window=win)
    t_got, t_z = pa.msm_execute_parallel(tabled, scalars)
    pre = pa.msm_precompute(c.curve_id, bases, 8, device_window=win, table_free=True)
    assert tabled.window == win and pre.window == win
    for run in range(2):   # the context is reusable
        got, gz = pa.msm_execute_parallel(pre, scalars)
        if not _same(got, gz, exp, ez):
            pytest.fail("table-free MSM, %s, window %d, execution %d (the tabled context is %s): %s"
                        % (c.name, win, run, "right" if _same(t_got, t_z, exp, ez) else "wrong too", _localise(c, pre, pool, logs, None)))
    assert _same(t_got, t_z, exp, ez), "the tabled context (no split) is wrong, the table-free one is right"
    # one vector of a batch of three
    outs, ozs = pa.msm_execute_batch(pre, np.stack([mont_arr(c.scalar, [0] * n), scalars, mont_arr(c.scalar, [r - 1] * n)]))
    assert int(ozs[0]) == 1 and _same(outs[1], ozs[1], exp, ez)
    assert _same(outs[2], ozs[2], *_multiple(c, -sum(logs)))
    # an identity among the generators (under a tie plant where the pool has it in k1) and generator 5 = generator 4
    flags = np.zeros(n, dtype=np.uint8)
    flags[ks.index(gh.find(pool, "k1:tie").k)] = 1
    bases[5], logs[5] = bases[4], logs[4]
    pre2 = pa.msm_precompute(c.curve_id, bases, 8, zero=flags, device_window=win, table_free=True)
    got, gz = pa.msm_execute_parallel(pre2, scalars)
    if not _same(got, gz, *_multiple(c, _dot(ks, logs, flags))):
        pytest.fail("table-free MSM with an identity and a repeated generator, %s, window %d: %s" % (c.name, win, _localise(c, pre2, pool, logs, flags)))
    for ctx in (tabled, pre, pre2):
        ctx.free()


def _fold_cases(c):
    """m = 6 pairs of known multiples of G: P == Q, Q == -P, identity lo, identity hi, two ordinary pairs"""
    m = 6
    pts, logs = _bases(c, 2 * m)
    lo, hi, llo, lhi = pts[:m].copy(), pts[m:].copy(), logs[:m], logs[m:]
    hi[0], lhi[0] = lo[0], llo[0]
    hi[1], lhi[1] = _pt(c, br.ec_neg(c, tuple(from_mont_arr(c.base, lo[1])))), -llo[1]
    lz, hz = np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.uint8)
    lz[2] = hz[3] = 1
    return lo, hi, llo, lhi, lz, hz


def _fold_all(c, lo, hi, lz, hz):
    return [pa.fold_generators(c.curve_id, lo, hi, mont_arr(c.scalar, [a])[0], mont_arr(c.scalar, [b])[0], lo_zero=lz, hi_zero=hz)
            for _, a, b in gh.fold_scalar_pairs(c.curve_id)]


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pair_fold_on_chosen_halves(c, monkeypatch):
    """out_i = [a] lo_i + [b] hi_i for the scalar pairs of fold_scalar_pairs (forms of lengths 1 against 130, 0 against 126, the longest on
    both sides, a negative half beside a tie plant) against integers - and the same words from the kernel without the split"""
    lo, hi, llo, lhi, lz, hz = _fold_cases(c)
    with_split = _fold_all(c, lo, hi, lz, hz)
    for (label, a, b), (got, gz) in zip(gh.fold_scalar_pairs(c.curve_id), with_split):
        for i in range(len(llo)):
            exp, ez = _multiple(c, (0 if lz[i] else a * llo[i]) + (0 if hz[i] else b * lhi[i]))
            assert int(gz[i]) == ez and (ez or np.array_equal(got[i], exp)), (c.name, label, i)
    monkeypatch.setenv("PLK_FOLD_NO_GLV", "1")   # read at every call
    for (label, _, _), (got, gz), (got2, gz2) in zip(gh.fold_scalar_pairs(c.curve_id), with_split, _fold_all(c, lo, hi, lz, hz)):
        live = gz == 0
        assert np.array_equal(gz, gz2) and np.array_equal(got[live], got2[live]), (c.name, label)


@pytest.mark.parametrize("r_bits,n_out,start", [(1, 1, 0), (1, 5, 3), (2, 1, 0), (2, 5, 2), (4, 1, 0), (4, 5, 0)])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_multi_fold_on_chosen_halves(c, r_bits, n_out, start):
    """out_i = g_i + sum_t [s_t] g_{i + t n_out} with the T - 1 scalars from the pool (tie, carry chain, longest halves, the chain on a
    negative k2, a (K, 0) split first), stored at the bit-reversed positions; an identity input and a repeated point among the g"""
    torch = pytest.importorskip("torch")
    from plonky_amd import device as dev
    dev.init(0)
    f = c.scalar
    T = 1 << r_bits
    n = T * n_out
    picks = gh.multi_fold_scalars(c.curve_id, T - 1, start)
    assert len(picks) == T - 1
    s = [0] + [m.k for m in picks]
    g, logs = _bases(c, n)
    g[n - 1], logs[n - 1] = g[0], logs[0]
    zero = np.zeros(n, dtype=np.uint8)
    if n > 2:
        zero[n // 2] = 1
    rev = lambda t: int(format(t, "0%db" % r_bits)[::-1], 2)
    sc = np.zeros((T, 4), dtype=np.uint64)
    for t in range(1, T):
        sc[rev(t)] = f.mont_limbs(s[t])
    out, oz = dev.fold_generators_multi_dev(c.curve_id, dev.to_device(g), dev.to_device(sc), r_bits, g_zero=torch.from_numpy(zero).cuda())
    out, oz = dev.to_host(out), oz.cpu().numpy()
    for i in range(n_out):
        k = (0 if zero[i] else logs[i]) + sum(s[t] * logs[i + t * n_out] for t in range(1, T) if not zero[i + t * n_out])
        exp, ez = _multiple(c, k)
        assert int(oz[i]) == ez and (ez or np.array_equal(out[i], exp)), (c.name, [m.label for m in picks], i)


def test_halo_round_with_a_planted_challenge():
    """one round of the inner-product argument on Tweedledum whose challenge u splits into a negative second half that is one carry chain"""
    pytest.importorskip("torch")
    from plonky_amd import device as dev
    dev.init(0)
    c = br.TWEEDLEDUM
    f = c.scalar
    n = 8
    plant = gh.negative_k2_plant(gh.half_pool(c.curve_id, gh.FOLD_WINDOW))
    assert plant.label == "k2-:chain" and plant.k2 < 0
    u, u_inv = mont_arr(f, [plant.k])[0], mont_arr(f, [pow(plant.k, -1, f.p)])[0]
    g, _ = _bases(c, n)
    a, b = ol.rand_field(f.field_id, 0x6171, n), ol.rand_field(f.field_id, 0x6172, n)
    a2, b2, g2, gz2 = dev.halo_round_fold_dev(c.curve_id, dev.to_device(a), dev.to_device(b), dev.to_device(g), u, u_inv)
    ea, eb, eg, egz = ol.halo_round_fold(c.curve_id, f.field_id, a, b, g, u, u_inv)
    assert np.array_equal(dev.to_host(a2), ea) and np.array_equal(dev.to_host(b2), eb)
    assert np.array_equal(gz2.cpu().numpy(), egz) and np.array_equal(dev.to_host(g2), eg)
