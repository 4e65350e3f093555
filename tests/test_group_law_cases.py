"""CPU-only: the case table of the group-law tests (tests/group_law_cases.py) is what it says it is.

The expectations the GPU test holds plk_curve_op to come from bigint_ref; here every one of them is recomputed by the oracle's C++
restatement of the reference (affine_add / scalar_mul of oracle_lib, which shares nothing with bigint_ref) from the same operands, the
operands themselves are checked to be the multiples of G they claim to be, and the classes the table promises are counted, so that a
later edit cannot thin one out unnoticed.  The 2-torsion cases of BLS12-377 are outside the oracle (the reference never meets such a
point): they are checked against the curve equation and the group law only."""
import numpy as np
import pytest

from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from tests import group_law_cases as glc
from tests.test_oracle_kats import mont_arr

CURVES = list(br.CURVES.values())
MIN_PER_CLASS = 8


def _aff(c, P):
    xy, zero = glc.points_to_arrays(c, [P])
    return xy[0], int(zero[0])


def _same(c, got, P):
    xy, zero = got
    exy, ez = _aff(c, P)
    return zero == ez and np.array_equal(xy, exy)


def _scalar(c, k):
    return mont_arr(c.scalar, [k % c.scalar.p])[0]


def _has_t(call):
    return any(o is not None and o.k == glc.T for e in call.elements for o in (e.a, e.b))


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_operands_are_the_multiples_they_claim(c):
    G = np.array([c.base.mont_limbs(c.gx), c.base.mont_limbs(c.gy)], dtype=np.uint64)
    seen = set()
    for call in glc.calls(c.curve_id):
        assert 1 <= len(call.elements) <= glc.MAX_ELEMENTS
        for e in call.elements:
            for o in (e.a, e.b):
                if o is None or o.k == glc.T:
                    continue
                assert abs(o.k) < 1 << 20 and 0 < o.lam < c.base.p
                seen.add(o.k)
    assert 64 <= len({abs(k) for k in seen if k}) <= 70   # the pool
    for k in sorted(seen):
        P = glc.point(c.curve_id, k)
        assert br.ec_on_curve(c, P)
        assert _same(c, ol.scalar_mul(c.curve_id, _scalar(c, k), G), P), k


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_expected_values_equal_the_oracle(c):
    cid = c.curve_id
    add = lambda A, B: ol.affine_add(cid, A[0], A[1], B[0], B[1])
    checked = 0
    for call in glc.calls(cid):
        if _has_t(call):
            continue
        pts = lambda which: [None if getattr(e, which) is None else _aff(c, glc.point(cid, getattr(e, which).k)) for e in call.elements]
        A, B = pts("a"), pts("b")
        if call.op == "wave_sum_q":
            assert len(call.expected) == -(-len(A) // call.param)
            for g, exp in enumerate(call.expected):
                s = _aff(c, None)
                for P in A[g * call.param:(g + 1) * call.param]:
                    s = add(s, P)
                assert _same(c, s, exp), (call.op, call.param, g)
                checked += 1
            continue
        assert len(call.expected) == len(call.elements)
        for i, (e, exp) in enumerate(zip(call.elements, call.expected)):
            if call.op in ("add", "add_q", "madd"):
                got = add(A[i], B[i])
            elif call.op == "madd_entry":
                Bn = _aff(c, br.ec_neg(c, glc.point(cid, e.b.k))) if e.flags & glc.NEGATE else B[i]
                got = add(A[i], Bn)
            elif call.op in ("dbl", "dbl_q"):
                got = add(A[i], A[i])
            elif call.op == "dbl_q_times":
                assert call.param in glc.TIMES
                got = ol.scalar_mul(cid, _scalar(c, 1 << call.param), A[i][0], A[i][1])
            else:
                assert call.op == "chain_q"
                s = add(add(A[i], B[i]), A[i])
                got = add(s, s)
            assert _same(c, got, exp), (call.op, call.param, i, e)
            checked += 1
    assert checked > 3000


def test_two_torsion_cases_follow_the_group_law():
    c = br.BLS12_377
    T = glc.point(c.curve_id, glc.T)
    assert T == (c.base.p - 1, 0) and br.ec_on_curve(c, T) and br.ec_add(c, T, T) is None
    n = 0
    for call in glc.calls(c.curve_id):
        if not _has_t(call):
            continue
        for e, exp in zip(call.elements, call.expected):
            A = glc.point(c.curve_id, e.a.k)
            if e.b is None:
                assert e.a.k == glc.T and exp is None
            else:
                B = glc.point(c.curve_id, e.b.k)
                if e.flags & glc.NEGATE:
                    B = br.ec_neg(c, B)
                if e.a.k == glc.T and e.b.k == glc.T:
                    assert exp is None
                else:
                    # exp = A + B: on the curve, not an operand, and exp - B = A, exp - A = B
                    assert exp is not None and br.ec_on_curve(c, exp) and exp not in (A, B)
                    assert br.ec_add(c, exp, br.ec_neg(c, B)) == A and br.ec_add(c, exp, br.ec_neg(c, A)) == B
            n += 1
    assert n == 2 * 16 + 4 * 48
    for other in CURVES:
        if other is not c:
            assert not any(_has_t(call) for call in glc.calls(other.curve_id))


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_every_class_is_there(c):
    n = glc.class_counts(c.curve_id)
    want = []
    for inflated in (False, True):
        for law in (glc.ONE_LANE, glc.QUAD):
            want += [(law, cls, inflated) for cls in glc.PAIR_CLASSES]
            want += [(law, "identity", inflated)]                               # doubling the identity
            if c is br.BLS12_377:
                want += [(law, cls, inflated) for cls in glc.T_CLASSES]
        want += [(glc.QUAD, "times_%d" % k, inflated) for k in glc.TIMES]
        want += [(glc.QUAD, "wave_" + w, inflated) for w in glc.WAVE_CLASSES]
        want += [(glc.QUAD, "b_is_minus_2a", inflated)]
    for key in want:
        assert n[key] >= MIN_PER_CLASS, (key, n[key])
    calls = glc.calls(c.curve_id)
    # the two operands of an element never share a lambda; lambdas 1, 2 and p - 1 occur
    lams = set()
    for call in calls:
        for e in call.elements:
            lams.add(e.a.lam)
            if e.b is not None and call.op not in ("madd", "madd_entry"):
                assert e.a.lam != e.b.lam
    assert {1, 2, c.base.p - 1} <= lams and len(lams) > 100
    # the ragged lengths, per operation that takes them
    for op in ("add", "add_q", "madd", "madd_entry", "dbl", "dbl_q", "chain_q"):
        assert sorted(len(call.elements) for call in calls if call.op == op and not _has_t(call)) == sorted(glc.LENGTHS), op
    assert {call.param for call in calls if call.op == "dbl_q_times"} == set(glc.TIMES)
    waves = [call for call in calls if call.op == "wave_sum_q"]
    assert [call.param for call in waves] == list(glc.GROUPS)
    q16 = waves[-1]
    equal16 = [g for g in range(len(q16.expected)) if q16.elements[16 * g].cls == "equal" and len({e.a.k for e in q16.elements[16 * g:16 * g + 16]}) == 1]
    assert len(equal16) >= MIN_PER_CLASS   # 16 equal points: every level of the wave sum doubles
    assert any(len(call.elements) % call.param for call in waves)   # a short last group
