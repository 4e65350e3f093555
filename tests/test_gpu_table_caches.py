"""GPU tests of the cache of device-resident tables (plonky_amd/csrc/table_cache.h) through the entry points that use it: the NTT plans,
the Plonk and Plookup circuit-size tables, the geometric tables and the z_H tables of poly.hip.  Every result is compared with the
oracle call the family's own test uses, at the smallest sizes the entry points take: what is under test is who owns the tables and
when they are rebuilt, not the kernels."""
import random
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import plonky_amd as pa
from plonky_amd import api, lib, synth
from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from tests import plookup_ref as pr
from tests.test_gpu_permutation import random_case, to_dev_args, z_restated
from tests.test_oracle_plonk import mont, unmont

F = br.TWEEDLEDEE_BASE
ZH_CACHE_MAX_ENTRIES = 64  # poly.hip


def clear():
    lib.check(lib.load().plk_ntt_clear_cache())


def transform_case():
    x = synth.rand_field(F.field_id, 0x7AB1E, 4)
    want = ol.FftPrecomputation(F.field_id, 4).fft_with_precomputation_power_of_2(x)
    return (lambda: pa.fft_with_precomputation_power_of_2(x, pa.fft_precompute(F.field_id, 4))), (lambda got: np.array_equal(got, want))


def permutation_case(log_n=1, seed=0x7AB2E):
    w, s_full, k, beta, gamma = random_case(F, log_n, seed, 1)
    want, _ = z_restated(F, log_n, w, s_full, k, beta, gamma)
    args = to_dev_args(F, w, s_full, k, beta, gamma)
    return (lambda: api.permutation_polynomial(F.field_id, 1 << log_n, *args, sigma_stride=1)), (lambda got: unmont(F, got) == want)


def plookup_case():
    rng = random.Random(0x7AB3E)
    log_size, p = 1, F.p
    rows = [[rng.randrange(p) for _ in range(4 << log_size)] for _ in range(5)]
    scalars = [rng.randrange(p) for _ in range(3)]
    want = pr.vanishing_values(F, log_size, *rows, *scalars)
    rm = np.stack([mont(F, r) for r in rows])
    sc = [mont(F, [v])[0] for v in scalars]
    return (lambda: api.plookup_vanishing_values(F.field_id, rm, *sc)), (lambda got: unmont(F, got) == want)


def mul_case():
    a, b = synth.rand_field(F.field_id, 0x7AB4E, 3), synth.rand_field(F.field_id, 0x7AB5E, 2)
    want = ol.poly_mul(F.field_id, a, b)
    return (lambda: pa.polynomial_mul(F.field_id, a, b)), (lambda got: np.array_equal(got, want))


def z_h_case():
    m = synth.rand_field(F.field_id, 0x7AB6E, 5)
    want = ol.poly_divide_by_z_h(F.field_id, m, 2)
    return (lambda: pa.polynomial_divide_by_z_h(F.field_id, m, 2)), (lambda got: np.array_equal(got, want))


@pytest.mark.parametrize("case", [transform_case, permutation_case, plookup_case, mul_case, z_h_case], ids=lambda c: c.__name__)
def test_clear_then_rebuild(case):
    """one call, plk_ntt_clear_cache, the same call: the tables are built, dropped and built again, and both results are the oracle's"""
    run, is_oracles = case()
    first = run()
    clear()
    second = run()
    assert is_oracles(first) and is_oracles(second)


def test_z_h_cache_bound():
    """One polynomial, 66 distinct n: two more tables than the z_H cache keeps, so the smallest keys are dropped along the way, and the
    first three n again (rebuilt: each of them pushes another table out).  No non-zero polynomial of 16 coefficients is a multiple of
    66 different X^n - 1, so the division that is exact here is the one the oracle makes - a(x) / (x^n - 1) at the 16 points
    x = g w^i of the coset, interpolated: it is defined for the n below because no denominator is zero, which is checked first."""
    a = synth.rand_field(F.field_id, 0x7AB7E, 16)
    ns = list(range(1, ZH_CACHE_MAX_ENTRIES + 3))
    assert len(set(ns)) == 66 > ZH_CACHE_MAX_ENTRIES
    p, g, w = F.p, F.generator, F.primitive_root_of_unity(4)
    points = [g * pow(w, i, p) % p for i in range(16)]
    assert all(pow(x, n, p) != 1 for n in ns for x in points)
    want = {n: ol.poly_divide_by_z_h(F.field_id, a, n) for n in ns}
    assert all(q.shape == (16, 4) for q in want.values())
    clear()
    for n in ns + ns[:3]:
        assert np.array_equal(pa.polynomial_divide_by_z_h(F.field_id, a, n), want[n]), n


def test_first_build_from_four_threads():
    """after a clear, four threads ask for the tables of one size at once: one of them builds, the others find them"""
    run, is_oracles = permutation_case(log_n=4, seed=0x7AB8E)
    clear()
    results, errors = [None] * 4, []
    start = threading.Barrier(4)

    def work(i):
        try:
            start.wait()
            results[i] = run()
        except BaseException as e:  # noqa: BLE001 - reported below, on the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(np.array_equal(r, results[0]) for r in results[1:])
    assert is_oracles(results[0])
