"""GPU parity: the point arithmetic of the MSM kernels against big integers, operation by operation.

plk_curve_op runs ONE operation of ecz.cuh (the one-lane law: xyzzz_add, xyzzz_dbl, the lazy mixed addition behind xyzzz_madd and
xyzzz_madd_entry) or of ecz_coop.cuh (the quad law: xyzzz_add_q, xyzzz_dbl_q, wave_sum_q - what every tail kernel of msm.hip and
msm_tail.hip runs on) per element and hands the result back in affine form, which is unique: every comparison is bit for bit with
bigint_ref's ec_add / ec_mul on the same operands (tests/group_law_cases.py; tests/test_group_law_cases.py checks that table against the
oracle on the host).  The table presents what the MSM tests on random generators never do: A = B and A = -B through different XYZZ
representatives, identity operands on either side, operands at the upper end of the accumulator invariant (X + 6p, Y + 2p), repeated
doublings, wave sums in which every level doubles or cancels, quad results fed back into the quad law, and on BLS12-377 the 2-torsion
point (p - 1, 0).  All lanes of a quad must hold the same result: the mismatch word of every call is 0 - the quad broadcast
(quad_bcast_u32) carries a workaround for a compiler fault that showed exactly there.

The library's own self-test of the quad law against the one-lane law (plk_selftest_quad) runs on every curve as well, down to ONE point,
where both of its indices fall together and its addition case becomes a doubling."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from plonky_amd import api, lib as plk
from tests import group_law_cases as glc

CURVES = list(br.CURVES.values())


@pytest.fixture(scope="module", autouse=True)
def _device():
    from plonky_amd import device as dev
    dev.init(0)


def _run(c, call):
    a = glc.operand_arrays(c, call, "a")
    b = glc.operand_arrays(c, call, "b")
    if b is not None and call.op in ("madd", "madd_entry"):
        b = (b[0], b[1], None)   # the affine operand has no lambda
    return api.curve_op(c.curve_id, call.op, a, b, glc.flag_array(call), call.param)


def _wrong(c, call, out, zero):
    """indices of the results that differ from the table's"""
    exy, ez = glc.points_to_arrays(c, list(call.expected))
    assert out.shape == exy.shape and zero.shape == ez.shape
    return [i for i in range(len(call.expected)) if int(zero[i]) != int(ez[i]) or not np.array_equal(out[i], exy[i])]


@pytest.mark.parametrize("law", [glc.ONE_LANE, glc.QUAD])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_point_operations_match_big_integers(c, law):
    failures = []
    for n, call in enumerate(glc.calls(c.curve_id)):
        if glc.LAW[call.op] != law:
            continue
        out, zero, mismatch = _run(c, call)
        bad = _wrong(c, call, out, zero)
        if bad or mismatch:
            i = bad[0] if bad else None
            el = None if i is None else (call.elements[i * call.param:(i + 1) * call.param] if call.op == "wave_sum_q" else call.elements[i])
            failures.append((n, call.op, call.param, len(call.elements), "mismatch word %d" % mismatch, "%d wrong results" % len(bad), i, el))
    for f in failures:
        print(f)
    assert not failures, failures[0]


def test_the_table_reaches_the_device_as_it_is():
    """the same identity in, the same identity out, and a result where the table has one: the wrapper's arrays are the table's"""
    c = br.TWEEDLEDEE
    call = next(k for k in glc.calls(c.curve_id) if k.op == "add" and len(k.elements) == 65)
    out, zero, mismatch = _run(c, call)
    assert mismatch == 0 and out.shape == (65, 2, 4)
    both = [i for i, e in enumerate(call.elements) if e.cls == "id_both"]
    assert both and all(zero[i] == 1 and not out[i].any() for i in both)
    plain = [i for i, e in enumerate(call.elements) if e.cls == "ordinary"]
    assert plain and all(zero[i] == 0 and out[i].any() for i in plain)


@pytest.mark.parametrize("op,param,count", [(9, 0, 4), (-1, 0, 4), (6, 0, 4), (6, 25, 4), (7, 3, 4), (7, 32, 4), (0, 0, 2049)])
def test_arguments_out_of_range_are_refused(op, param, count):
    buf = np.ones(2049 * 8, dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    mism = ctypes.c_uint(7)
    rc = plk.load().plk_curve_op(0, op, param, count, p, p, p, p, p, p, p, p, p, ctypes.byref(mism))
    assert rc == plk.PLK_ERR_INVALID_ARG


@pytest.mark.parametrize("n", [1, 2, 7, 64])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_quad_self_test_on_every_curve(c, n):
    """plk_selftest_quad: eight cases of the quad law against the one-lane law over 1024 quads on n points k G; with n = 1 the two
    indices of a quad coincide, so case 0 (an addition) is a doubling inside the addition.  All eight counters stay zero."""
    pts, _ = glc.points_to_arrays(c, [br.ec_mul(c, 3 + 5 * i, (c.gx, c.gy)) for i in range(n)])
    cnt = (ctypes.c_uint * 8)(*([0xFFFFFFFF] * 8))
    plk.check(plk.load().plk_selftest_quad(c.curve_id, pts.ctypes.data_as(ctypes.c_void_p), n, 1024, cnt))
    assert list(cnt) == [0] * 8
