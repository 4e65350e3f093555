"""CPU-only: the case table of the plain XYZZ law's tests (tests/xyzz_cases.py) is what it says it is.

The replay of k_sum_affine's schedule must give, for every case, the sum big integers name from the multiples alone; every case must
reach the (site, branch, lane) it was built for, the tree's doubling and cancelling cases with two different non-affine representatives;
the labels are listed here once more, so that a builder cannot leave the table unnoticed, and together the aims hit every (site, branch)
pair of the law.  The exchange records of the combine cases are taken apart again byte by byte and their expected values recomputed by
plain point additions."""
import numpy as np
import pytest

from oracle import bigint_ref as br
from tests import xyzz_cases as xc

CURVES = list(br.CURVES.values())


def _names(case):
    return [e for e in case.entries if e not in (xc.FLAG, xc.JUNK)]


@pytest.fixture(scope="module")
def replays():
    return {c.curve_id: {case.label: xc.schedule(c.curve_id, case.entries) for case in xc.sum_cases(c.curve_id)} for c in CURVES}


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_the_replay_gives_the_sum_of_the_multiples(c, replays):
    G = (c.gx, c.gy)
    identities = 0
    for case in xc.sum_cases(c.curve_id):
        got, steps = replays[c.curve_id][case.label]
        names = _names(case)
        assert all(abs(k) <= xc.MAX_K for k, _ in names)
        k, t = sum(n[0] for n in names), sum(n[1] for n in names) % 2
        want = br.ec_mul(c, k % c.scalar.p, G)   # G has the order of the scalar field
        if t:
            want = br.ec_add(c, want, (c.base.p - 1, 0))
        assert got == want == xc.named_sum(c.curve_id, names) and br.ec_on_curve(c, got), case.label
        assert len([s for s in steps if s.site == "madd"]) == len(names) and len(steps) == len(names) + 63
        identities += got is None
    assert identities >= 8   # among them the lists that cancel as a whole, all-flagged and the empty one


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_every_case_reaches_what_it_was_built_for(c, replays):
    for case in xc.sum_cases(c.curve_id):
        _, steps = replays[c.curve_id][case.label]
        at = {(s.site, s.branch, s.lane): s for s in steps if s.site != "madd"}
        madds = {(s.site, s.branch, s.lane) for s in steps if s.site == "madd"}
        for aim in case.aims:
            assert aim in at or aim in madds, (case.label, aim)
            if aim[0] != "madd" and aim[1] in ("double", "cancel"):
                # both lane sums were formed from two points: neither is affine any more, and they are two representatives
                s = at[aim]
                assert s.a[2] != 1 and s.b[2] != 1 and s.a != s.b and s.a[2] != s.b[2], case.label
                if aim[1] == "double":
                    assert xc.rep_to_affine(c.base.p, s.a) == xc.rep_to_affine(c.base.p, s.b)
        if case.label.startswith("madd/double") or case.label.startswith("madd/cancel"):
            s = next(s for s in steps if (s.site, s.branch, s.lane) == case.aims[0])
            assert s.a is not None and s.b[2:] == (1, 1)


def _expected_labels(c):
    ends = lambda d: sorted({0, d - 1})
    labels = ["madd/double@0", "madd/double@63", "madd/cancel@0", "madd/cancel@63", "madd/after-flag@0", "madd/after-flag@63",
              "madd/after-junk", "all-flagged"]
    labels += ["add@%d/%s@%d" % (d, b, t) for d in xc.DS for b in ("double", "cancel") for t in ends(d)]
    labels += ["add@%d/%s" % (d, b) for d in xc.DS for b in ("left-identity", "right-identity")]
    labels += ["size-%d" % k for k in (0, 1, 2, 63, 64, 65, 127, 128, 129, 193)]
    if c is br.BLS12_377:
        labels += ["T+T", "T+T+P", "add@32/double-T", "add@1/double-T"]
    return labels


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_the_cover_is_complete(c):
    cases = xc.sum_cases(c.curve_id)
    assert sorted(case.label for case in cases) == sorted(_expected_labels(c))
    aimed = {aim[:2] for case in cases for aim in case.aims}
    want = {("madd", b) for b in ("left-identity", "generic", "double", "cancel")}
    want |= {("add@%d" % d, b) for d in (32, 16, 8, 4, 2, 1) for b in ("left-identity", "right-identity", "generic", "double", "cancel")}
    assert aimed == want == set(xc.PAIRS)
    # the collisions sit at the first and at the last lane of their level
    lanes = {}
    for case in cases:
        for site, branch, lane in case.aims:
            if branch in ("double", "cancel"):
                lanes.setdefault((site, branch), set()).add(lane)
    assert lanes[("madd", "double")] >= {0, 63} and lanes[("madd", "cancel")] >= {0, 63}
    for d in xc.DS:
        for b in ("double", "cancel"):
            assert lanes[("add@%d" % d, b)] >= {0, d - 1}
    # flagged slots that hold no curve point, and a list of nothing else
    by = {case.label: case for case in cases}
    assert xc.JUNK in by["madd/after-junk"].entries and not _names(by["all-flagged"]) and xc.JUNK in by["all-flagged"].entries
    xy, zero = xc.sum_arrays(c, by["madd/after-junk"])
    assert zero[0] == 1 and (xy[0] == 0xFFFFFFFFFFFFFFFF).all() and zero[64] == 0 and zero[2] == 1 and not xy[2].any()
    assert [len(by["size-%d" % k].entries) for k in xc.SIZES] == list(xc.SIZES)


def test_two_torsion_names():
    c = br.BLS12_377
    Tp = xc.point(c.curve_id, xc.T)
    assert Tp == (c.base.p - 1, 0) and br.ec_on_curve(c, Tp) and br.ec_add(c, Tp, Tp) is None
    A, B = xc.point(c.curve_id, xc.P(21)), xc.point(c.curve_id, xc.t_minus(21))
    assert br.ec_on_curve(c, B) and br.ec_add(c, A, B) == Tp and xc.neg(xc.T) == xc.T
    for other in CURVES:
        if other is not c:
            assert not any(e not in (xc.FLAG, xc.JUNK) and e[1] for case in xc.sum_cases(other.curve_id) for e in case.entries)
            assert not any(e not in (xc.FLAG, xc.JUNK) and e[1] for case in xc.combine_cases(other.curve_id) for row in case.cells for e in row)


# ---------------------------------------------------------------------------------------------
# combine cases
# ---------------------------------------------------------------------------------------------
def test_combine_geometries():
    assert xc.WORLDS == (1, 2, 3, 4, 5, 7, 8, 64, 65, 130)
    for world in xc.WORLDS:
        g = {name: (batch, whole) for name, batch, whole in xc.geometries(world)}
        for batch, whole in g.values():
            assert whole * world <= batch and xc.slots_of(world, batch, whole) >= 5
        assert g["sharded"][1] == 0
        assert g["whole"][0] == g["whole"][1] * world
        assert g["below-floor"][1] < g["below-floor"][0] // world
        mods = {batch % world for name, (batch, whole) in g.items() if name.startswith("hybrid") and whole == batch // world and batch % world}
        assert mods == {m for m in (1, 2, world - 1) if 0 < m < world}, world


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_combine_records_and_expected_values(c):
    L = c.base.n_limbs
    contents, checked, decoded = set(), 0, {}
    for case in xc.combine_cases(c.curve_id):
        w, gname, content = case.label.split("/")
        contents.add((case.world <= 8, content))
        slots = xc.slots_of(case.world, case.batch, case.whole)
        rec, pts = xc.record_bytes(c, slots), slots * 2 * L * 8
        assert rec % 16 == 0 and pts + slots <= rec < pts + slots + 16
        buf, expected = xc.combine_layout(case)
        assert buf.dtype == np.uint8 and buf.shape == (case.world * rec,) and len(expected) == case.batch
        rows = buf.reshape(case.world, rec)
        assert (rows[:, pts + slots:] == 0xFF).all()
        flags = rows[:, pts:pts + slots]
        words = rows[:, :pts].copy().view(np.uint64).reshape(case.world, slots, 2, L)
        for r in range(case.world):
            for s in range(slots):
                e = case.cells[r][s]
                assert flags[r, s] == (1 if e == xc.FLAG else 0)
                if e in (xc.FLAG, xc.JUNK):
                    assert (words[r, s] == 0xFFFFFFFFFFFFFFFF).all()
                else:
                    key = words[r, s].tobytes()
                    if key not in decoded:   # the same few thousand points fill every case
                        decoded[key] = tuple(c.base.from_mont(br.limbs_to_int([int(w) for w in words[r, s, i]])) for i in (0, 1))
                    assert decoded[key] == xc.point(c.curve_id, e)
        if content == "checker":   # a set flag has clear neighbours and a clear flag set ones
            assert (flags[:, 1:] != flags[:, :-1]).all()
        # a naive sum per vector
        for v in range(case.batch):
            if v < case.whole * case.world:
                cells = [case.cells[v % case.world][v // case.world]]
            else:
                cells = [case.cells[r][case.whole + v - case.whole * case.world] for r in range(case.world)]
            if xc.JUNK in cells:
                assert expected[v] == xc.UNCHECKED and content == "junk-beside-whole"
                continue
            acc = None
            for e in cells:
                if e != xc.FLAG:
                    acc = br.ec_add(c, acc, xc.point(c.curve_id, e))
            assert expected[v] == acc, (case.label, v)
            if content == "all-flagged":
                assert acc is None
            checked += 1
        if content == "junk-beside-whole" and case.whole:
            assert any(e != xc.UNCHECKED for e in expected[:case.whole * case.world]) and xc.UNCHECKED in expected or case.world == 1
    small = {k for s, k in contents if s}
    assert small >= set(xc.SMALL_CONTENTS) and {k for s, k in contents if not s} == set(xc.BIG_CONTENTS)
    assert ("T-two" in small) == (c is br.BLS12_377)
    assert checked > 3000


def test_colliding_ranks_share_a_lane_of_the_stride_loop():
    case = next(k for k in xc.combine_cases(0) if k.label == "w130/sharded/collide-64")
    col = [row[0] for row in case.cells]
    assert col[64] == col[0] and col[65] == xc.neg(col[1]) and col[129] not in (xc.FLAG, xc.JUNK)
    case = next(k for k in xc.combine_cases(0) if k.label == "w65/sharded/collide-64")
    assert case.cells[64][0] == case.cells[0][0]
