"""CPU-only: the restatement tests/halo_endo_ref.py against itself on the four curves with the endomorphism - the reference's own
test_halo_n ([halo_n(bits)] P == halo_n_mul(bits, P)), phi(P) = [ZETA_SCALAR] P, and the order of `us` in halo_g."""
import pytest

from oracle import bigint_ref as br
from tests import halo_endo_ref as he


@pytest.mark.parametrize("curve", he.ENDO_CURVES)
def test_endomorphism_is_multiplication_by_zeta_scalar(curve):
    c = br.CURVES[curve]
    assert pow(he.zeta(curve), 3, c.base.p) == 1 and he.zeta(curve) != 1
    assert pow(he.zeta_scalar(curve), 3, c.scalar.p) == 1 and he.zeta_scalar(curve) != 1
    for k in (1, 2, 12345):
        P = br.ec_mul(c, k, (c.gx, c.gy))
        assert br.ec_on_curve(c, he.endomorphism(curve, P))
        assert he.endomorphism(curve, P) == br.ec_mul(c, he.zeta_scalar(curve), P)


@pytest.mark.parametrize("curve", he.ENDO_CURVES)
@pytest.mark.parametrize("security_bits", (2, 4, 128, "max"))
def test_halo_n_mul_is_multiplication_by_halo_n(curve, security_bits):
    c = br.CURVES[curve]
    bits = (c.scalar.bits & ~1) if security_bits == "max" else security_bits
    P = br.ec_mul(c, 0xC0FFEE, (c.gx, c.gy))
    seen = set()
    for s in he.chunk_patterns(bits, seed=curve + 1):
        sb = he.bits_of(s, bits)
        seen.update((pos, sb[2 * pos] | sb[2 * pos + 1] << 1) for pos in (0, bits // 4, bits // 2 - 1))
        assert br.ec_mul(c, he.halo_n(curve, sb), P) == he.halo_n_mul(curve, sb, P), hex(s)
    assert len(seen) == 4 * len({0, bits // 4, bits // 2 - 1})
    assert he.halo_n_mul(curve, he.bits_of(5, bits), None) is None


def test_halo_n_small_cases():
    # one chunk: (lo, hi) = (1, 0) -> b = 1, (0, 0) -> b = -1, (1, 1) -> a = 1, (0, 1) -> a = -1
    for curve in he.ENDO_CURVES:
        r, z = br.CURVES[curve].scalar.p, he.zeta_scalar(curve)
        assert [he.halo_n(curve, he.bits_of(s, 2)) for s in range(4)] == [r - 1, 1, (r - z) % r, z]
        # two chunks: the first chunk is doubled
        assert he.halo_n(curve, [1, 0, 1, 1]) == (2 + z) % r


@pytest.mark.parametrize("field", (0, 1, 4, 5))
@pytest.mark.parametrize("k", (1, 3, 5))
def test_halo_g_is_the_folded_b(field, k):
    """halo_g(x, us) equals what is left of b = powers(x) after the folds of halo.rs:118 with us[0] first: this pins the order of us."""
    p = br.FIELDS[field].p
    gen = br.splitmix64_stream(100 + field + k)
    x = next(gen) * next(gen) % p
    us = [(next(gen) << 64 | next(gen)) % p or 1 for _ in range(k)]
    b = [pow(x, i, p) for i in range(1 << k)]
    for u in us:
        b = he.fold_b(p, b, u)
    assert b == [he.halo_g(p, x, us)]
    if k > 1:
        assert he.halo_g(p, x, us[::-1]) != b[0]
