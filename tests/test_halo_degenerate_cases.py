"""The case table of tests/halo_degenerate_cases.py against the oracle (no GPU): on every family, at n = 8 and n = 16, on all five
curves, the closed form on logarithms must give the words and flags of ol.halo_round_lr / ol.halo_round_fold wherever those accept
the inputs (no identity among the generators), and of their composition from ol.MsmPrecomputation(..., zero=), ol.scalar_mul and
ol.affine_add where there are flags.  The planned identity positions, the families and the family / regime exceptions are asserted
too: a table that lost a case, or a case that stopped reaching its branch, fails here before it reaches a device."""
import numpy as np
import pytest

from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from tests import halo_degenerate_cases as hd

CURVES = [br.TWEEDLEDEE, br.TWEEDLEDUM, br.BLS12_377, br.PALLAS, br.VESTA]


def _same(got_xy, got_z, want_xy, want_z):
    """the oracle's identity carries whatever coordinates the reference leaves: there the flag alone is compared"""
    return int(got_z) == int(want_z) and (want_z or np.array_equal(got_xy, want_xy))


def _oracle_lr(c, a, b, g, gz, h, up, l_blind, r_blind, ips):
    """halo_round_lr (halo.rs:86-93) with identity flags on the generators"""
    m = a.shape[0] // 2
    outs = []
    for a_half, g_half, z_half, blind, ip in ((a[:m], g[m:], gz[m:], l_blind, ips[0]), (a[m:], g[:m], gz[:m], r_blind, ips[1])):
        xy, z = ol.MsmPrecomputation(c.curve_id, g_half, 8, zero=z_half).execute(a_half, parallel=True)
        t1, z1 = ol.scalar_mul(c.curve_id, blind, h)
        t2, z2 = ol.scalar_mul(c.curve_id, ip, up)
        xy, z = ol.affine_add(c.curve_id, xy, z, t1, z1)
        outs.append(ol.affine_add(c.curve_id, xy, z, t2, z2))
    return outs


def _oracle_fold_g(c, g, gz, u, u_inv):
    m = g.shape[0] // 2
    out, oz = [], []
    for i in range(m):
        p1, z1 = ol.scalar_mul(c.curve_id, u_inv, g[i], gz[i])
        p2, z2 = ol.scalar_mul(c.curve_id, u, g[m + i], gz[m + i])
        xy, z = ol.affine_add(c.curve_id, p1, z1, p2, z2)
        out.append(xy)
        oz.append(z)
    return np.stack(out), np.array(oz, dtype=np.uint8)


def check_case_against_oracle(case, closed_form=hd.closed_form):
    c, f = case.c, case.c.scalar
    g, gz, h, up, a, b, us, blind = hd.case_arrays(case)
    p = f.p
    ai, bi = list(case.a), list(case.b)
    direct = 0
    for j, rd in enumerate(closed_form(case)):
        m = a.shape[0] // 2
        what = "%s (%s) n %d round %d" % (case.name, c.name, case.n, j)
        u_inv = hd.scalar_words(c, [pow(case.us[j], -1, p)])[0]
        want = [hd.point_words(c, rd.L), hd.point_words(c, rd.R)]
        if not gz.any():
            exp, ez = ol.halo_round_lr(c.curve_id, f.field_id, a, b, g, h, up, blind[2 * j], blind[2 * j + 1])
            got = list(zip(exp, ez))
            direct += 1
        else:
            ips = hd.scalar_words(c, [sum(ai[i] * bi[m + i] for i in range(m)), sum(ai[m + i] * bi[i] for i in range(m))])
            got = _oracle_lr(c, a, b, g, gz, h, up, blind[2 * j], blind[2 * j + 1], ips)
        for q, (gxy, gzf), (wxy, wz) in zip("LR", got, want):
            assert _same(gxy, gzf, wxy, wz), "%s: %s" % (what, q)
        if not gz.any():
            a2, b2, g2, gz2 = ol.halo_round_fold(c.curve_id, f.field_id, a, b, g, us[j], u_inv)
        else:
            a2, b2, _, _ = ol.halo_round_fold(c.curve_id, f.field_id, a, b, np.tile(h, (2 * m, 1, 1)), us[j], u_inv)   # the scalar halves of the fold
            g2, gz2 = _oracle_fold_g(c, g, gz, us[j], u_inv)
        assert np.array_equal(a2, hd.scalar_words(c, rd.a)) and np.array_equal(b2, hd.scalar_words(c, rd.b)), "%s: a / b" % what
        for i in range(m):
            wxy, wz = hd.point_words(c, rd.k[i])
            assert _same(g2[i], gz2[i], wxy, wz), "%s: g[%d]" % (what, i)
        a, b, g, gz, ai, bi = a2, b2, g2, np.asarray(gz2, dtype=np.uint8), rd.a, rd.b
    return direct


@pytest.mark.parametrize("n", [8, 16])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_closed_form_matches_the_oracle(c, n):
    direct = sum(check_case_against_oracle(case) for case in hd.build_cases(c, n))
    assert direct >= 10 * (n.bit_length() - 1)   # most families have no flag: ol.halo_round_lr / ol.halo_round_fold themselves


@pytest.mark.parametrize("n", [8, 16, 64])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_every_family_is_there_and_reaches_its_positions(c, n):
    cases = hd.build_cases(c, n)   # asserts planned == found for every case
    rounds = n.bit_length() - 1
    by_family = {fam: [case for case in cases if case.family == fam] for fam in hd.FAMILIES}
    assert sorted(len(v) for v in by_family.values()) == [1, 2, 2, 3, 4, 5, 5] and len({case.name for case in cases}) == len(cases) == 22
    assert all(case.family in hd.FAMILIES and case.branch for case in cases)
    named = {case.name: case for case in cases}
    every = {("g", j, i) for j in range(rounds) for i in range(n >> (j + 1))}
    m = n // 2
    # the planned positions, restated: a table whose builders and `identities` drifted together would still meet these
    assert named["flagged_pair"].planned == {("g", 0, 1)} and named["flagged_corners"].planned == {("g", 0, 0), ("g", 0, m - 1)}
    assert not named["flagged_lo_edges"].planned and not named["flagged_hi_edges"].planned and not named["flagged_quarter"].planned
    assert sum(named["flagged_quarter"].flags) == n // 4 and named["flagged_quarter"].flags[-1] and named["flagged_hi_edges"].flags[m]
    for case in by_family["flagged"]:
        idx = [i for i in range(n) if case.flags[i]]
        assert len(case.decoy) == len(idx) // 2 and all(case.decoy[i] for i in case.decoy)   # half zero words, half a valid point
    assert named["fold_all"].planned == every == named["fold_equal_halves"].planned
    assert named["fold_some_round0"].planned == {("g", 0, 0), ("g", 0, m - 1), ("g", 0, m // 2), ("g", 1, 0)}
    assert named["fold_some_round1"].planned == {("g", 1, m // 2 - 1)} | ({("g", 1, 0)} if n >= 16 else set())
    assert named["all_zero"].planned == {(q, j) for j in range(rounds) if j != 1 for q in "LR"}
    assert named["cancelled"].planned == {("LR"[j % 2], j) for j in range(rounds)}
    for name in ("one_point", "opposite_first", "opposite_every_round", "a_zero", "a_lo_zero", "b_zero", "special_u_forward", "special_u_backward",
                 "h_equals_u", "u_minus_h", "h_in_upper_half"):
        assert not named[name].planned, name
    # the special challenges are what they are called, and both orders together cover all four at every n
    p = c.scalar.p
    i, w = hd.sqrt_minus_one(p), hd.cube_root_of_unity(p)
    seen = set(named["special_u_forward"].us) | set(named["special_u_backward"].us)
    assert {1, p - 1, i, w} <= seen and i * i % p == p - 1 and w != 1 and pow(w, 3, p) == 1
    assert named["fold_equal_halves"].us[0] == i and named["fold_equal_halves"].k[:m] == named["fold_equal_halves"].k[m:]
    assert named["opposite_every_round"].a[:m] == named["opposite_every_round"].a[m:]
    assert named["h_equals_u"].k_h == named["h_equals_u"].k_u and (named["u_minus_h"].k_h + named["u_minus_h"].k_u) % p == 0
    assert named["h_in_upper_half"].k_h == named["h_in_upper_half"].k[n - 1]


def test_family_regime_exceptions():
    """no family is excused from a regime of tests/test_gpu_halo_degenerate.py"""
    assert hd.EXCEPTIONS == []


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_points_by_logarithm_match_double_and_add(c):
    p = c.scalar.p
    for k in (1, 2, 3, hd.K_P, p - 1, p - hd.K_P, (p - 1) // 2, 1 << (p.bit_length() - 1), p - (1 << (p.bit_length() - 1)), 0x9E3779B97F4A7C15 ** 3 % p):
        assert hd.point(c, k) == br.ec_mul(c, k, (c.gx, c.gy)), hex(k)
    assert hd.point(c, 0) is None and hd.point(c, p) is None and hd.point_words(c, 0)[1] == 1 and not hd.point_words(c, 0)[0].any()
