"""GPU parity of the inner-product argument's context (plk_halo_*) on degenerate inputs, against a closed form.

tests/test_gpu_halo.py draws generic inputs: distinct generators, random scalars, no identity flags - no fold ever produces an
identity there, no L_j / R_j is one, and d_halo_g_zero never reaches the rebind, the freeze, the in-place scaled fold, the 2^r-to-1
fold or the caller's tables.  Here every point is a known multiple of the curve's generator (tests/halo_degenerate_cases.py, held
against the oracle by tests/test_halo_degenerate_cases.py), so every L_j, R_j, halo_a, halo_b, halo_g and flag of every round is
arithmetic on Python integers and one point by its logarithm - compared bit for bit; an identity counts only as flag 1 with all-zero
words.  Every family runs through every regime of the context at the smallest size at which the regime exists, by the protocol of
test_gpu_halo._run_argument (round_lr twice per round, len after every fold, read(with_g=not frozen) after every fold, a final read).
The rounds that report `frozen` are asserted per regime: a case cannot pass by taking another regime."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from tests import checked_child
from tests import halo_degenerate_cases as hd
from tests.test_gpu_halo import _run_argument

ENDO = (br.TWEEDLEDEE, br.TWEEDLEDUM, br.PALLAS, br.VESTA)
F, T = False, True
# id -> (n, freeze_log, environment, arguments of _run_argument, curves, `frozen` after every fold: with / without the endomorphism)
REGIMES = {
    # pairwise folds 16 -> 8 -> 4 -> 2, frozen when two generators are left (the smallest freeze_log)
    "pairwise": (16, 1, {}, {}, (br.TWEEDLEDEE, br.PALLAS, br.BLS12_377), ([F, F, T, T],) * 2),
    "frozen_comb": (16, 0, {}, {}, (br.TWEEDLEDEE, br.PALLAS, br.BLS12_377), ([T, T, T, T],) * 2),
    "frozen_buckets": (16, 0, {"PLK_MSM_COMB": "0"}, {}, (br.TWEEDLEDEE, br.BLS12_377), ([T, T, T, T],) * 2),
    "frozen_part_way": (64, 3, {}, {}, ENDO + (br.BLS12_377,), ([F, F, T, T, T, T],) * 2),
    # one stage of two virtual rounds over the explicit set (64 -> 16 by the 4-to-1 fold), a pairwise fold, frozen at 8
    "virtual_stages": (64, 3, {"PLK_HALO_STAGE_MIN_LOG": "1"}, {}, ENDO, ([T, F, T, T, T, T], None)),
    # two lead rounds over the caller's tables (65 generators, H / U' from the pair kernel), pairwise folds 16 -> 8 -> 4, frozen at 4
    "lead_hu_beside": (64, 2, {}, dict(tabled=True, lead_rounds=2, extra_generators=1), (br.TWEEDLEDEE, br.PALLAS), ([T, F, F, T, T, T], None)),
    # ... H and U are generators 65 and 66 of the tables; BLS12-377 has no endomorphism and falls back to pairwise folds from the start
    "lead_hu_inside": (64, 2, {}, dict(tabled=True, lead_rounds=2, extra_generators=1, inside=True), (br.TWEEDLEDEE, br.PALLAS, br.BLS12_377),
                       ([T, F, F, T, T, T], [F, F, F, T, T, T])),
}
PARAMS = [pytest.param(rid, c, id="%s-%s" % (rid, c.name)) for rid, r in REGIMES.items() for c in r[4]]
ENV = ("PLK_MSM_COMB", "PLK_HALO_STAGE_MIN_LOG", "PLK_HALO_STAGE", "PLK_HALO_FREEZE_LOG", "PLK_HALO_LEAD")


def _point_diff(c, got_xy, got_z, log):
    """None, or what is wrong with a point whose logarithm is known"""
    want_xy, want_z = hd.point_words(c, log)
    if int(got_z) != want_z:
        return "flag %d, expected %d" % (int(got_z), want_z)
    if not np.array_equal(np.asarray(got_xy).reshape(want_xy.shape), want_xy):
        return "identity with non-zero words" if want_z else "wrong words"
    return None


def _case_failures(rid, case):
    """one case through one regime -> the list of everything that differs from the closed form"""
    n, freeze_log, _, kw, _, frozen_by_endo = REGIMES[rid]
    c = case.c
    want_frozen = frozen_by_endo[0 if c is not br.BLS12_377 else 1]
    g, gz, h, up, a, b, us, blind = hd.case_arrays(case)
    where = "%s / %s / %s / %s" % (rid, c.name, case.family, case.name)
    tail = " [built for: %s]" % case.branch
    try:
        _, lrs, states, (fa, fb, fg, fgz) = _run_argument(c, n, freeze_log, 0, g_zero=gz if gz.any() else None, inputs=(g, h, up, a, b, us, blind),
                                                          inside_u=hd.inside_u(case) if kw.get("inside") else None, **kw)
    except AssertionError as e:   # round_lr called twice gave two answers, or a wrong length after a fold
        return ["%s: the protocol of _run_argument: %r%s" % (where, e, tail)]
    bad = []
    rounds = hd.closed_form(case)
    if [s[0] for s in states] != want_frozen:
        bad.append("%s: took another regime: frozen after the folds %r, expected %r" % (where, [s[0] for s in states], want_frozen))
    for j, (rd, (lr, z), (frozen, got)) in enumerate(zip(rounds, lrs, states)):
        for q, t, log in (("L", 0, rd.L), ("R", 1, rd.R)):
            d = _point_diff(c, lr[t], z[t], log)
            if d:
                bad.append("%s: round %d: %s: %s" % (where, j, q, d))
        for q, arr, vals in (("a", got[0], rd.a), ("b", got[1], rd.b)):
            if not np.array_equal(arr, hd.scalar_words(c, vals)):
                bad.append("%s: round %d: halo_%s after the fold" % (where, j, q))
        if not frozen:
            for i, log in enumerate(rd.k):
                d = _point_diff(c, got[2][i], got[3][i], log)
                if d:
                    bad.append("%s: round %d: g[%d] after the fold: %s" % (where, j, i, d))
    last = rounds[-1]
    if not (np.array_equal(fa, hd.scalar_words(c, last.a)) and np.array_equal(fb, hd.scalar_words(c, last.b))):
        bad.append("%s: final halo_a / halo_b" % where)
    d = _point_diff(c, fg[0], fgz[0], last.k[0])
    if d:
        bad.append("%s: final halo_g: %s" % (where, d))
    return [line + tail for line in bad]


def _regime_failures(rid, c, families=hd.FAMILIES):
    n = REGIMES[rid][0]
    cases = [case for case in hd.build_cases(c, n) if case.family in families]
    assert {case.family for case in cases} == set(families)   # no family is dropped for a regime
    return [line for case in cases for line in _case_failures(rid, case)], len(cases)


@pytest.mark.parametrize("rid,c", PARAMS)
def test_degenerate_inputs_match_the_closed_form(rid, c, monkeypatch):
    pytest.importorskip("torch")
    from plonky_amd import device as dev
    dev.init(0)
    for name in ENV:   # read when an argument begins / when a context is built
        monkeypatch.delenv(name, raising=False)
    for name, value in REGIMES[rid][2].items():
        monkeypatch.setenv(name, value)
    bad, count = _regime_failures(rid, c)
    assert count == 22
    assert not bad, "\n".join(bad)   # every family runs, so that a failure lists all the families it shows in


# ---- the checked build: the flagged generators and the identities made by a fold, pairwise and frozen, every guard counter zero ----
def run_checked_cases():
    count = 0
    for c in (br.TWEEDLEDEE, br.BLS12_377):
        for rid in ("pairwise", "frozen_comb"):
            bad, k = _regime_failures(rid, c, ("flagged", "fold_identities"))
            assert not bad, "\n".join(bad)
            count += k
    return count


CHECKED_BODY = '''
from plonky_amd import device as dev
dev.init()
from tests.test_gpu_halo_degenerate import run_checked_cases
print("CHECKED compared", run_checked_cases())
'''


def test_checked_build_flags_and_fold_identities():
    assert "CHECKED compared 36" in checked_child.run_checked(CHECKED_BODY)
