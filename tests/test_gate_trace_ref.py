"""CPU-only: the restatement of the two gadgets (tests/gate_trace_ref.py) held to judges that share nothing with it: the oracle's
evaluate_all_constraints (oracle/plonk_gates.inc) is zero in all eight terms on every block row, with the constants the restatement
writes; the Rescue block's last row is rescue_ref's permutation; the curve_msm result minus 2^(n_bits - 1) start is the sum of s_j P_j
on integers; the exceptional cases and the overrun are counted and written as include/plonky_hip_trace.h says."""
import numpy as np
import pytest

from oracle import bigint_ref as br, oracle_lib as ol
from tests import gate_trace_cases as gc
from tests import gate_trace_ref as gt
from tests import rescue_ref as rr

N_ROWS = 64  # below = row + 65 wraps to row + 1


def assert_block_rows_satisfied(field, wires, constants, rows):
    f = br.FIELDS[field]
    w, k = gt.table(f, wires, 9, N_ROWS), gt.table(f, constants, 6, N_ROWS)
    zero = np.zeros(4, dtype=np.uint64)
    for i in rows:
        terms = ol.gate_constraints(field, -1, k[:, i], w[:, i], w[:, (i + 1) % N_ROWS], w[:, (i + 65) % N_ROWS], zero, zero)
        assert terms.shape == (8, 4) and not terms.any(), (field, i, terms)


@pytest.mark.parametrize("field", gc.RESCUE_FIELDS)
def test_rescue_blocks_satisfy_the_gates_and_end_on_the_permutation(field):
    f = br.FIELDS[field]
    rounds = 3
    consts = rr.constants(field, 4, rounds)
    v = gc.values(f, 0x51 + field, 8)
    inputs = [v[:4], [0, 0, 0, 0], v[4:]]
    block = gt.rescue_block_rows(rounds)
    first = [2, 2 + block, N_ROWS - block]  # back to back, and one that ends on the last row
    wires, constants, status = gt.trace_rescue(field, inputs, consts, N_ROWS, first)
    assert status == [0, 0, gt.NONE, 0]
    assert_block_rows_satisfied(field, wires, constants, [r + i for r in first for i in range(block)])
    for state, r in zip(inputs, first):
        assert [wires[(i, r + 2 * rounds)] for i in range(4)] == rr.rescue_permutation(field, state, consts)
        assert [wires[(i, r)] for i in range(4)] == list(state)
        assert all(pow(wires[(4 + i, r)], 5, f.p) == state[i] for i in range(4))
        assert all((j, r + i) not in wires for i in range(block) for j in ((8,) if i % 2 == 0 and i < 2 * rounds else range(4, 9)))
    assert [constants[(j, first[0] + 2 * rounds)] for j in range(6)] == [1, 0, 1, 0, 0, 0]
    # one row too few: the block is refused whole
    w2, k2, s2 = gt.trace_rescue(field, inputs[:1], consts, N_ROWS, [N_ROWS - block + 1])
    assert (w2, k2, s2) == ({}, {}, [1, 0, gt.NONE, 0])


@pytest.mark.parametrize("curve", gc.MSM_CURVES)
@pytest.mark.parametrize("parts,n_bits", [(1, 1), (2, 5), (3, 4)])
def test_curve_msm_blocks_satisfy_the_gates_and_sum_the_parts(curve, parts, n_bits):
    c = br.CURVES[curve]
    start = gc.start_point(curve)
    pts = gc.points(curve, 3 * parts + n_bits, 2 * parts)
    rnd = [v % (1 << n_bits) for v in gc.values(c.base, 0xA0 + curve, 2 * parts)]
    scs = [rnd[:parts], ([0, (1 << n_bits) - 1, 1] * 3)[:parts]]
    block = gt.msm_block_rows(parts, n_bits)
    first = [1, N_ROWS - block]
    wires, constants, status = gt.trace_curve_msm(curve, [pts[:parts], pts[parts:]], scs, start, n_bits, N_ROWS, first)
    assert status == [0, 0, gt.NONE, 0]
    assert_block_rows_satisfied(c.base.field_id, wires, constants, [r + i for r in first for i in range(block)])
    for p, s, r in zip([pts[:parts], pts[parts:]], scs, first):
        assert gc.msm_result(curve, wires, r, parts, n_bits, start) == gc.msm_sum(curve, p, s)
        assert all(br.ec_on_curve(c, (wires[(0, r + i)], wires[(1, r + i)])) for i in range(block))
        for j in range(parts):  # each part's accumulator ends on its scalar (circuit_curve.rs:405-407)
            assert wires[(3, r + (n_bits - 1) * (parts + 1) + j)] == s[j]


@pytest.mark.parametrize("curve", gc.MSM_CURVES)
def test_curve_msm_exceptional_cases(curve):
    c = br.CURVES[curve]
    start = gc.start_point(curve)
    parts, n_bits = 2, 4
    pts = gc.points(curve, 9, 2)
    scs = [0b1011, 0b0011]
    block = gt.msm_block_rows(parts, n_bits)
    mid = gc.x_collision_point(curve, pts, scs, start, n_bits, 1, 1)  # bit 1, part 1: block row 2 * 3 + 1
    cases = [([start, pts[1]], scs, 0), ([pts[0], mid], scs, 7), (pts, [0b1011, 1 << n_bits], 0), ([pts[0], br.ec_neg(c, mid)], scs, 7)]
    first = gc.back_to_back(len(cases), block) + [N_ROWS]
    wires, constants, status = gt.trace_curve_msm(curve, [p for p, _, _ in cases] + [pts], [s for _, s, _ in cases] + [scs], start, n_bits, N_ROWS, first)
    assert status == [1, len(cases), 0, 0]
    for (p, s, stop), r in zip(cases, first):
        for i in range(block):
            defined = 9 if i % (parts + 1) < parts else 6
            row = [wires[(w, r + i)] for w in range(defined)]
            assert (not any(row)) == (i >= stop), (stop, i)
            assert [constants[(j, r + i)] for j in range(5)] == ([1, 0, 1, 0, 1] if defined == 9 else [1, 0, 1, 1, 1])
    # the rows before the stop still satisfy their gates, up to the one whose right neighbour was zeroed
    ok_rows = [first[1] + i for i in range(6)]
    assert_block_rows_satisfied(c.base.field_id, wires, constants, ok_rows)
