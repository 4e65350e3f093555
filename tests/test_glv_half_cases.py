"""What the pools of tests/glv_half_cases.py must hold, stated on the restated recodings alone (no GPU): the conditions that keep the
comparisons of tests/test_gpu_glv_paths.py from passing vacuously.  Every (curve, window) pool is judged by the digits
restated_half_digits gives its halves, not by how a member was built."""
import pytest

from oracle import bigint_ref as br
from tests import glv_half_cases as gh
from tests.scalar_mul_cases import GLV_BITS, glv_params, glv_split

CASES = [(cv, c) for cv in gh.ENDO_CURVES for c in gh.WINDOWS]
IDS = ["%s-c%d" % (br.CURVES[cv].name, c) for cv, c in CASES]
K2_NEGATIVE = (1, 4)      # Tweedledum, Vesta: B2 < 0, the second half of a random scalar is negative
K2_POSITIVE = (0, 3)      # Tweedledee, Pallas


def test_restated_half_digits_on_small_cases():
    """the rule itself on values worked out by hand, c = 3 (half = 4): 4 is the tie (stays 4, no carry), 5 is the first negative
    digit (-3, carry), 7 + carry = 8 has no entry and carries on, and a negative half flips every digit"""
    w = gh.windows_of(3)
    pad = lambda d: d + [0] * (w - len(d))
    assert w == 44 and gh.windows_of(10) == 14 and gh.windows_of(13) == 11 and gh.windows_of(16) == 9
    assert gh.restated_half_digits(0o4, 3) == pad([4])
    assert gh.restated_half_digits(0o5, 3) == pad([-3, 1])
    assert gh.restated_half_digits(0o775, 3) == pad([-3, 0, 0, 1])
    assert gh.restated_half_digits(-0o775, 3) == pad([3, 0, 0, -1])
    assert gh.restated_half_digits(-0o44, 3) == pad([-4, -4])
    assert gh.half_profile(0o775, 3) == (0, 1, 2) and gh.half_profile(-0o444, 3) == (3, 0, 0)


@pytest.mark.parametrize("curve,c", CASES, ids=IDS)
def test_pool_members_split_as_recorded(curve, c):
    r, lam = br.CURVES[curve].scalar.p, glv_params(curve)["LAMBDA"]
    pool = gh.half_pool(curve, c)
    assert 55 <= len(pool) <= 90
    for m in pool:
        assert glv_split(curve, m.k) == (m.k1, m.k2) and (m.k1 + m.k2 * lam - m.k) % r == 0, m.label
        assert abs(m.k1) < 1 << GLV_BITS and abs(m.k2) < 1 << GLV_BITS, m.label
        for h in (m.k1, m.k2):
            d = gh.restated_half_digits(h, c)
            assert len(d) == gh.windows_of(c) and sum(x << (c * j) for j, x in enumerate(d)) == h, m.label
    for want in ("0", "1", "r-1", "lambda", "r-lambda", "edge0", "rand31"):
        assert gh.find(pool, want), want


@pytest.mark.parametrize("curve,c", CASES, ids=IDS)
def test_pool_holds_every_pattern_in_both_halves(curve, c):
    pool, w = gh.half_pool(curve, c), gh.windows_of(c)
    for which, halves in (("k1", [m.k1 for m in pool]), ("k2", [m.k2 for m in pool])):
        prof = [gh.half_profile(h, c) for h in halves]
        assert max(p[0] for p in prof) >= w - 2, (which, "tie digits")
        assert max(p[1] for p in prof) >= w - 2, (which, "digits -(2^(c-1) - 1)")
        assert max(p[2] for p in prof) >= 3, (which, "consecutive windows without an entry that carry on")
    # the restated digits themselves, not only the walk: a tie is +-2^(c-1), and a negative half shows it negated
    half = 1 << (c - 1)
    for pick in (lambda m: m.k1, lambda m: m.k2):
        assert any(sum(abs(d) == half for d in gh.restated_half_digits(pick(m), c)) >= w - 2 for m in pool)
    assert any(m.k2 == 0 and m.k1.bit_length() >= 126 for m in pool)
    assert any(max(abs(m.k1), abs(m.k2)).bit_length() >= 129 for m in pool)


@pytest.mark.parametrize("curve,c", [cs for cs in CASES if cs[0] in K2_NEGATIVE], ids=[i for cs, i in zip(CASES, IDS) if cs[0] in K2_NEGATIVE])
def test_patterns_on_a_negative_second_half(curve, c):
    """Tweedledum and Vesta: the sign flip of the digits is reached through k2, and with every pattern"""
    pool, w, half = gh.half_pool(curve, c), gh.windows_of(c), 1 << (c - 1)
    prof = [gh.half_profile(m.k2, c) for m in pool if m.k2 < 0]
    assert max(p[0] for p in prof) >= w - 2 and max(p[1] for p in prof) >= w - 2 and max(p[2] for p in prof) >= 3
    assert any(sum(d == -half for d in gh.restated_half_digits(m.k2, c)) >= w - 2 for m in pool)              # flipped ties
    assert any(sum(d == half - 1 for d in gh.restated_half_digits(m.k2, c)) >= w - 2 for m in pool if m.k2 < 0)  # flipped first negative digits


@pytest.mark.parametrize("curve,c", CASES, ids=IDS)
def test_the_split_is_one_sided(curve, c):
    """The quotients of the split are floors, so a half is f1 (a1, b1) + f2 (a2, b2) with 0 <= f < 1: k1 is never negative (a1, a2 > 0),
    and k2 lies between b1 and b2, which have opposite signs and very different lengths (|b1| about 2^90, |b2| about 2^127).
    On Tweedledee and Pallas (b1 < 0 < b2) a negative half is therefore a k2 no lower than b1 - which lambda itself has (and r - 1 on Pallas),
    and which the builder's search reaches with the carry chains cut below 2^90: those members stay in the pool, they take the sign flip
    on these two curves.  No member has a negative half of any other kind; none of the whole-length patterns sits on one.  On
    Tweedledum and Vesta (b2 < 0 < b1) it is the positive k2 that stays below b1.  If gen_glv_params.py is re-run and picks another
    basis, this is the test that says so."""
    g, pool = glv_params(curve), gh.half_pool(curve, c)
    assert g["A1"] > 0 and g["A2"] > 0 and g["B1"] * g["B2"] < 0 and abs(g["B1"]).bit_length() <= 90 and abs(g["B2"]).bit_length() == 127
    assert (g["B1"] < 0) == (curve in K2_POSITIVE)
    assert not [m.label for m in pool if m.k1 < 0]
    lo, hi = min(g["B1"], g["B2"]), max(g["B1"], g["B2"])
    assert all(lo <= m.k2 <= hi for m in pool)
    if curve in K2_POSITIVE:
        neg = [m for m in pool if m.k2 < 0]
        assert all(m.k2 >= g["B1"] for m in neg)
        assert {m.label for m in neg} - {"lambda", "r-1"} == {m.label for m in pool if m.label.startswith("k2-:chain")} and gh.find(pool, "lambda") in neg
        assert not {"k2-:tie", "k2-:near", "k2-:chain"} & {m.label for m in pool}
        assert all(max(gh.half_profile(m.k2, c)[:2]) < gh.windows_of(c) - 2 for m in neg)
    else:
        pos = [m for m in pool if m.k2 > 0]
        assert all(m.k2 <= g["B1"] for m in pos)
        assert not {"k2+:tie", "k2+:near", "k2+:chain"} & {m.label for m in pool}
        assert sum(m.k2 < 0 for m in pool if m.label.startswith("rand")) == 32


@pytest.mark.parametrize("curve", gh.ENDO_CURVES, ids=lambda cv: br.CURVES[cv].name)
def test_top_window(curve):
    """c = 10 and c = 13: the top window starts at bit 130 and the halves have at most 129 bits (and a 129-bit half gives no carry into it:
    its last full window is below 2^(c-1)), so the window stays empty.  c = 16: the top window starts at bit 128 and is occupied."""
    for c in (10, 13):
        assert (gh.windows_of(c) - 1) * c == 130
        for m in gh.half_pool(curve, c):
            assert max(abs(m.k1), abs(m.k2)).bit_length() <= 129
            assert gh.restated_half_digits(m.k1, c)[-1] == 0 and gh.restated_half_digits(m.k2, c)[-1] == 0, m.label
    assert (gh.windows_of(16) - 1) * 16 == 128
    assert any(abs(gh.restated_half_digits(h, 16)[-1]) == 1 for m in gh.half_pool(curve, 16) for h in (m.k1, m.k2))


def _check_jsf(a, b):
    cols = gh.restated_jsf(a, b)
    assert sum(u << j for j, (u, _) in enumerate(cols)) == a and sum(v << j for j, (_, v) in enumerate(cols)) == b
    assert all(u in (-1, 0, 1) and v in (-1, 0, 1) for u, v in cols)
    assert not cols or cols[-1] != (0, 0)
    for j in range(len(cols) - 1):
        # Solinas: of any three consecutive columns one is empty, and two adjacent non-zero digits in one row only above a column
        # whose other row is 0 and beside one whose other row is not
        if j + 2 < len(cols):
            assert (0, 0) in cols[j:j + 3], (hex(a), hex(b), j)
        for i in (0, 1):
            if cols[j][i] and cols[j + 1][i]:
                assert cols[j][1 - i] == 0 and cols[j + 1][1 - i] != 0, (hex(a), hex(b), j, i)
    return cols


def test_restated_jsf():
    assert gh.restated_jsf(0, 0) == [] and gh.restated_jsf(1, 0) == [(1, 0)] and gh.restated_jsf(0, 1) == [(0, 1)]
    assert gh.restated_jsf(3, 0) == [(-1, 0), (0, 0), (1, 0)] and gh.restated_jsf(7, 7) == [(-1, -1), (0, 0), (0, 0), (1, 1)]
    for a in range(64):
        for b in range(64):
            _check_jsf(a, b)
    nonzero = total = 0
    for curve in gh.ENDO_CURVES:
        for m in gh.half_pool(curve, gh.FOLD_WINDOW):
            cols = _check_jsf(abs(m.k1), abs(m.k2))
            assert len(cols) <= max(abs(m.k1), abs(m.k2)).bit_length() + 1
            if m.label.startswith("rand"):
                nonzero += sum(c != (0, 0) for c in cols)
                total += len(cols)
    assert 0.45 < nonzero / total < 0.55      # half of the columns are empty on average


@pytest.mark.parametrize("curve", gh.ENDO_CURVES, ids=lambda cv: br.CURVES[cv].name)
def test_fold_pairs_bring_forms_of_unequal_length(curve):
    """the pair fold aligns two joint sparse forms of lengths na and nb at the least significant column: the pairs bring na << nb, na >> nb,
    na = 0, the longest forms on both sides, and a negative half beside a tie plant"""
    pairs = gh.fold_scalar_pairs(curve)
    assert len(pairs) == 7
    lens = [gh.jsf_lengths(curve, a, b) for _, a, b in pairs]
    assert any(nb - na >= 100 for na, nb in lens) and any(na - nb >= 100 for na, nb in lens)
    assert any(na == 0 for na, _ in lens) and any(min(na, nb) >= 129 for na, nb in lens)
    assert max(max(l) for l in lens) <= 131
    neg = gh.negative_k2_plant(gh.half_pool(curve, gh.FOLD_WINDOW))
    assert neg.k2 < 0 and gh.half_profile(neg.k2, gh.FOLD_WINDOW)[2] >= 3 and any(a == neg.k for _, a, _ in pairs)
    if curve in K2_NEGATIVE:
        assert neg.label == "k2-:chain" and abs(neg.k2).bit_length() == 125
    picks = gh.multi_fold_scalars(curve, 15)
    assert len(picks) == 15 and len({m.k for m in picks}) == 15 and any(m.k2 < 0 for m in picks[:5]) and any(m.k2 == 0 for m in picks[:5])
