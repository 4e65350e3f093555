"""The gate witness rows on Python integers, restated from the reference's behaviour: the block of rows CircuitBuilder::rescue_permutation
lays down (circuit_builder.rs:931-970) as RescueStepAGate / RescueStepBGate generate them (rescue_a.rs:116-155, rescue_b.rs), and the
block of curve_msm (circuit_curve.rs:287-410) as CurveAddGate / CurveDblGate generate it (curve_add.rs:229-260, curve_dbl.rs:150-175).
Values are canonical integers; a result is what the library's entries write: {(wire, row): value}, {(constant column, row): value}
and the four status words of include/plonky_hip_trace.h.  table() lays such writes over Montgomery limbs."""
import numpy as np

from oracle import bigint_ref as br
from tests import rescue_ref as rr

NONE = 0xFFFFFFFF
NUM_WIRES, NUM_CONSTANTS = 9, 6
PREFIX = {"rescue_a": "00", "rescue_b": "01", "buffer": "101000", "curve_add": "10101", "curve_dbl": "10111"}  # the code's, not mod.rs's doc comment


def _prefix(constants, gate, row):
    for j, bit in enumerate(PREFIX[gate]):
        constants[(j, row)] = int(bit)


def rescue_block_rows(rounds):
    return 2 * rounds + 1


def msm_block_rows(parts, n_bits):
    return n_bits * (parts + 1)


def trace_rescue(field, inputs, consts, n_rows, first_rows):
    """inputs: states of 4 canonical values; consts: rescue_ref.constants(field, 4, rounds).  Exponent 5 only (the gates' exp_usize(5))."""
    assert rr.ALPHA[field] == 5
    p = br.FIELDS[field].p
    wires, constants, status = {}, {}, [0, 0, NONE, 0]
    for state, first in zip(inputs, first_rows):
        if first + rescue_block_rows(len(consts)) > n_rows:
            status[0] += 1
            continue
        state = list(state)
        for k, (step_a, step_b) in enumerate(consts):
            row = first + 2 * k
            roots = [rr.kth_root(p, x, 5) for x in state]  # rescue_a.rs:132
            for i in range(4):
                wires[(i, row)] = state[i]
                wires[(4 + i, row)] = roots[i]
                constants[(2 + i, row)] = step_a[i]
                constants[(2 + i, row + 1)] = step_b[i]
            _prefix(constants, "rescue_a", row)
            _prefix(constants, "rescue_b", row + 1)
            state = [(a + b) % p for a, b in zip(rr.apply_mds(p, roots), step_a)]  # rescue_a.rs:144-152: the B row's wires
            for i in range(4):
                wires[(i, row + 1)] = state[i]
            state = [(a + b) % p for a, b in zip(rr.apply_mds(p, [pow(x, 5, p) for x in state]), step_b)]
        last = first + 2 * len(consts)
        for i in range(4):
            wires[(i, last)] = state[i]
        _prefix(constants, "buffer", last)
    return wires, constants, status


def trace_curve_msm(curve, points, scalars, start, n_bits, n_rows, first_rows):
    """points[c][j] = (x, y), scalars[c][j] canonical integers of the BASE field, start = (x, y).  An instance that meets an exceptional
    case (a scalar bit at or above n_bits, x1 = x2 in an add row, y = 0 in a doubling) has its rows from that one on written as zero."""
    p = br.CURVES[curve].base.p
    wires, constants, status = {}, {}, [0, 0, NONE, 0]
    for c, (pts, scs, first) in enumerate(zip(points, scalars, first_rows)):
        parts = len(pts)
        if first + msm_block_rows(parts, n_bits) > n_rows:
            status[0] += 1
            continue
        dead = any(s >> n_bits for s in scs)
        (ax, ay), row = start, first
        for i in range(n_bits - 1, -1, -1):
            for j in range(parts):
                _prefix(constants, "curve_add", row)
                (x2, y2), bit, acc_old = pts[j], (scs[j] >> i) & 1, scs[j] >> (i + 1)
                dead = dead or (ax - x2) % p == 0  # curve_add.rs:244 "x_1 = x_2"
                if dead:
                    vals = [0] * 9
                else:
                    inv = pow(ax - x2, -1, p)
                    lam = (ay - y2) * inv % p
                    x3 = (lam * lam - ax - x2) % p
                    y3 = (lam * (ax - x3) - ay) % p
                    vals = [ax, ay, acc_old % p, (2 * acc_old + bit) % p, x2, y2, bit, inv, lam]
                    if bit:
                        ax, ay = x3, y3
                for w, v in enumerate(vals):
                    wires[(w, row)] = v
                row += 1
            _prefix(constants, "curve_dbl", row)
            dead = dead or ay % p == 0  # curve_dbl.rs:157 "y = 0"
            if dead:
                vals = [0] * 6
            else:
                inv = pow(2 * ay, -1, p)
                lam = 3 * ax * ax * inv % p  # InnerC::A = 0
                xn = (lam * lam - 2 * ax) % p
                yn = (lam * (ax - xn) - ay) % p
                vals = [ax, ay, xn, yn, inv, lam]
                ax, ay = xn, yn
            for w, v in enumerate(vals):
                wires[(w, row)] = v
            row += 1
        if dead:
            status[1] += 1
            status[2] = min(status[2], c)
    return wires, constants, status


def table(f, writes, columns, n_rows, base=None):
    """(columns, n_rows, 4) uint64 Montgomery limbs: `base` (or zeros) with the writes laid over it"""
    t = np.zeros((columns, n_rows, 4), dtype=np.uint64) if base is None else np.array(base, dtype=np.uint64).reshape(columns, n_rows, 4)
    if writes:
        keys = np.array(list(writes), dtype=np.int64)
        t[keys[:, 0], keys[:, 1]] = np.array([f.mont_limbs(v) for v in writes.values()], dtype=np.uint64)
    return t


def limbs(f, values):
    """canonical integers (any nesting) -> Montgomery limbs with a trailing axis of 4"""
    a = np.array(values, dtype=object)
    return np.array([f.mont_limbs(int(v)) for v in a.reshape(-1)], dtype=np.uint64).reshape(a.shape + (4,))
