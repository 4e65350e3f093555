"""GPU tests of the gate witness rows (include/plonky_hip_trace.h; gate_trace.hip k_trace_rescue / k_trace_msm): every table is compared
word for word with the restatement tests/gate_trace_ref.py laid over the sentinel the table was filled with before the call, so a
wire the gate does not define, a row outside the blocks and a block that would pass n_rows must keep their bytes.

Shapes.  Rescue: counts at the edges of a quad group (15 | 16 | 17 states), of a wave and of a workgroup of 64 states (63 | 64 | 65)
and over several workgroups (257); contexts of 1 and 10 rounds.  curve_msm: one instance per lane in workgroups of 64 (63 | 64 | 65,
257); parts 1, 2, 3, 8; n_bits 1, 2, 8 and BITS - 1.  The closed loops put both gadgets into one 2^10-row table and ask judges that
share nothing with the kernels: the witness check, plk_rescue_permutation_dev, plk_curve_scalar_mul_dev and the curve sums."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from plonky_amd import api, lib
from tests import checked_child
from tests import gate_trace_cases as gc
from tests import gate_trace_ref as gt
from tests import rescue_ref as rr

NONE = 0xFFFFFFFF
SENTINEL = 0x5E47155E47155E47  # no limb of a written element: a canonical element's top limb is below 2^62


def dev_module():
    pytest.importorskip("torch")
    from plonky_amd import device as dev
    dev.init(0)
    return dev


def sentinel(columns, n_rows):
    return np.full((columns, n_rows, 4), SENTINEL, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def rescue_context(field, rounds):
    consts = rr.constants(field, 4, rounds)
    return consts, api.RescueContext(field, np.array(rr.constants_limbs(field, consts), dtype=np.uint64))


def run_rescue_dev(dev, field, rounds, inputs, n_rows, first, with_constants=True):
    """the device entry over sentinel tables -> (wires, constants or None, status words) on the host"""
    import torch
    f = br.FIELDS[field]
    _, ctx = rescue_context(field, rounds)
    w = dev.to_device(sentinel(9, n_rows))
    k = dev.to_device(sentinel(6, n_rows)) if with_constants else None
    out, st = dev.trace_rescue_permutation_dev(ctx, dev.to_device(gt.limbs(f, inputs)), n_rows, torch.tensor(first, dtype=torch.int32, device="cuda"),
                                               wires=w, constants=k, status=True)
    assert out is w
    return dev.to_host(w), None if k is None else dev.to_host(k), st.cpu().numpy().view(np.uint32).tolist()


def assert_tables(f, got_w, got_k, wires, constants, n_rows):
    want = gt.table(f, wires, 9, n_rows, base=sentinel(9, n_rows))
    assert np.array_equal(got_w, want), np.argwhere((got_w != want).any(axis=2))[:8]
    if got_k is not None:
        want_k = gt.table(f, constants, 6, n_rows, base=sentinel(6, n_rows))
        assert np.array_equal(got_k, want_k), np.argwhere((got_k != want_k).any(axis=2))[:8]


@pytest.mark.parametrize("field", gc.RESCUE_FIELDS)
@pytest.mark.parametrize("rounds", [1, 10])
def test_rescue_rows_match_the_restatement(field, rounds):
    dev = dev_module()
    f = br.FIELDS[field]
    consts, _ = rescue_context(field, rounds)
    block = gt.rescue_block_rows(rounds)
    v = gc.values(f, 0x7000 + 16 * field + rounds, 4 * 257)
    inputs = [v[4 * c:4 * c + 4] for c in range(257)]
    inputs[3] = [0, 0, 0, 0]
    for count in (1, 15, 16, 17, 63, 64, 65, 257):
        if count in (15, 17, 63, 65):
            first, n_rows = gc.scattered(count, block, count)
        else:
            first, n_rows = gc.back_to_back(count, block, 2), count * block + 2  # the last block ends at row n_rows - 1
        wires, constants, status = gt.trace_rescue(field, inputs[:count], consts, n_rows, first)
        got_w, got_k, got_st = run_rescue_dev(dev, field, rounds, inputs[:count], n_rows, first, with_constants=count != 16)
        assert got_st == status == [0, 0, NONE, 0], count
        assert_tables(f, got_w, got_k, wires, constants, n_rows)
        if count == 64:  # the receiving rows are the permutation, by the entry that computes nothing else
            perm = dev.to_host(dev.rescue_permutation_dev(rescue_context(field, rounds)[1], dev.to_device(gt.limbs(f, inputs[:count]))))
            assert np.array_equal(got_w[:4, np.array(first) + 2 * rounds].transpose(1, 0, 2), perm)


@pytest.mark.parametrize("field", gc.RESCUE_FIELDS)
def test_rescue_overrun_zero_state_and_the_host_form(field):
    dev = dev_module()
    f = br.FIELDS[field]
    rounds = 2
    consts, ctx = rescue_context(field, rounds)
    block = gt.rescue_block_rows(rounds)
    v = gc.values(f, 0x7100 + field, 16)
    inputs = [[0, 0, 0, 0], v[:4], v[4:8], v[8:12], v[12:]]
    n_rows = 40
    first = [7, n_rows - block + 1, n_rows - block, 0xFFFFFFFE, 20]  # one row too many, ending on the last row, a row near 2^32
    wires, constants, status = gt.trace_rescue(field, inputs, consts, n_rows, first)
    assert status == [2, 0, NONE, 0]
    got_w, got_k, got_st = run_rescue_dev(dev, field, rounds, inputs, n_rows, [x - (1 << 32) if x >> 31 else x for x in first])
    assert got_st == status
    assert_tables(f, got_w, got_k, wires, constants, n_rows)
    # the host-pointer form: the caller's tables in place, the same words
    w, k = sentinel(9, n_rows), sentinel(6, n_rows)
    w2, k2, st = api.trace_rescue_permutation(ctx, gt.limbs(f, inputs), n_rows, first, wires=w, constants=k)
    assert np.shares_memory(w2, w) and np.shares_memory(k2, k) and st.tolist() == status
    assert_tables(f, w, k, wires, constants, n_rows)
    w3, k3, st3 = api.trace_rescue_permutation(ctx, gt.limbs(f, inputs), n_rows, first)
    assert k3 is None and np.array_equal(w3, gt.table(f, wires, 9, n_rows)) and st3.tolist() == status


def test_rescue_refusals_with_a_context():
    """the refusals that need a context, in their documented order, through both forms; a context over the exponent-11 field and over
    the six-limb field"""
    dev_module()
    L = lib.load()
    _, ctx = rescue_context(0, 1)
    got = gc.refusal_results(L, gc.ENTRIES[:2], gc.RESCUE_ORDER, gc.RESCUE_GOOD, gc.RESCUE_REFUSALS, ctx=ctx.handle)
    want = [r for _ in gc.ENTRIES[:2] for r in gc.RESCUE_REFUSALS]
    for (entry, name, code, text), (n, _, starts) in zip(got, want):
        assert name == n and code == lib.PLK_ERR_INVALID_ARG and text.startswith(starts), (entry, name, code, text)
    for field, starts in ((2, "field 2: Rescue exponent 11"), (3, "field 3 has 6 limbs")):
        consts = rr.constants(field, 4, 1)
        with api.RescueContext(field, np.array(rr.constants_limbs(field, consts), dtype=np.uint64)) as other:
            for override in (dict(), dict(n_rows=0, inputs=None)):
                res = gc.refusal_results(L, gc.ENTRIES[:2], gc.RESCUE_ORDER, gc.RESCUE_GOOD, [("ctx", override, starts)], ctx=other.handle)
                assert all(code == lib.PLK_ERR_INVALID_ARG and text.startswith(starts) for _, _, code, text in res), res
    assert L.plk_trace_rescue_permutation_dev(0, ctx.handle, None, 64, None, None, None, None, None) == lib.PLK_OK


# ---- curve_msm ----
def run_msm_dev(dev, curve, P, S, start, n_bits, n_rows, first, with_constants=True):
    import torch
    f = br.CURVES[curve].base
    w = dev.to_device(sentinel(9, n_rows))
    k = dev.to_device(sentinel(6, n_rows)) if with_constants else None
    out, st = dev.trace_curve_msm_dev(curve, dev.to_device(gt.limbs(f, P)), dev.to_device(gt.limbs(f, S)), gt.limbs(f, start), n_bits, n_rows,
                                      torch.tensor(first, dtype=torch.int32, device="cuda"), wires=w, constants=k, status=True)
    assert out is w
    return dev.to_host(w), None if k is None else dev.to_host(k), st.cpu().numpy().view(np.uint32).tolist()


def msm_inputs(curve, parts, n_bits, count, seed):
    """seeded points and scalars below 2^n_bits; the first instances take the scalars 0, 1 and 2^n_bits - 1 in every part"""
    f = br.CURVES[curve].base
    pts = gc.points(curve, seed, count * parts)
    rnd = [x % (1 << n_bits) for x in gc.values(f, 0x8800 + seed, count * parts)]
    P = [pts[i * parts:(i + 1) * parts] for i in range(count)]
    S = [rnd[i * parts:(i + 1) * parts] for i in range(count)]
    for i, s in enumerate((0, 1, (1 << n_bits) - 1)[:count]):
        S[i] = [s] * parts
    return P, S


@pytest.mark.parametrize("curve", gc.MSM_CURVES)
@pytest.mark.parametrize("parts,n_bits,count", [(1, 8, 257), (2, 2, 65), (3, 8, 64), (8, 1, 63), (8, 8, 5), (3, 2, 1), (2, None, 3)])
def test_curve_msm_rows_match_the_restatement(curve, parts, n_bits, count):
    dev = dev_module()
    c = br.CURVES[curve]
    n_bits = c.base.bits - 1 if n_bits is None else n_bits
    start = gc.start_point(curve)
    P, S = msm_inputs(curve, parts, n_bits, count, 31 * parts + n_bits + count)
    block = gt.msm_block_rows(parts, n_bits)
    if count in (63, 65):
        first, n_rows = gc.scattered(count, block, count)
    else:
        first, n_rows = gc.back_to_back(count, block, 1), count * block + 1
    wires, constants, status = gt.trace_curve_msm(curve, P, S, start, n_bits, n_rows, first)
    assert status == [0, 0, NONE, 0], "the seeded case must meet no exceptional case in the restatement itself"
    got_w, got_k, got_st = run_msm_dev(dev, curve, P, S, start, n_bits, n_rows, first, with_constants=count != 64)
    assert got_st == status
    assert_tables(c.base, got_w, got_k, wires, constants, n_rows)


@pytest.mark.parametrize("curve", gc.MSM_CURVES)
def test_curve_msm_planted_exceptions(curve):
    dev = dev_module()
    c = br.CURVES[curve]
    f, start = c.base, gc.start_point(curve)
    parts, n_bits = 2, 4
    pts = gc.points(curve, 9, 4)
    scs = [0b1011, 0b0011]
    block = gt.msm_block_rows(parts, n_bits)
    mid = gc.x_collision_point(curve, pts[:2], scs, start, n_bits, 1, 1)  # x1 = x2 first at bit 1, part 1: block row 7
    P = [pts[2:], [start, pts[1]], pts[:2], [pts[0], mid], pts[:2], pts[2:]]
    S = [scs, scs, scs, scs, [0b1011, 1 << n_bits], [5, 9]]
    n_rows = len(P) * block
    first = gc.back_to_back(len(P) - 1, block) + [n_rows - block + 1]  # the last one would pass the end
    wires, constants, status = gt.trace_curve_msm(curve, P, S, start, n_bits, n_rows, first)
    assert status == [1, 3, 1, 0]
    for c_i, stop in ((1, 0), (3, 7), (4, 0)):  # the restatement zeroes from the planted row on, and not before
        assert all(wires[(0, first[c_i] + i)] == 0 for i in range(stop, block)) and all(wires[(0, first[c_i] + i)] for i in range(stop))
    got_w, got_k, got_st = run_msm_dev(dev, curve, P, S, start, n_bits, n_rows, first)
    assert got_st == status
    assert_tables(f, got_w, got_k, wires, constants, n_rows)
    # the host-pointer form says which: the reference's panic text for the first such instance, the tables written all the same
    for order, exc, text in (([1, 0], AssertionError, "x_1 = x_2: instance 0, block row 0"), ([3, 0], AssertionError, "x_1 = x_2: instance 0, block row 7"),
                             ([4, 1], ValueError, "scalar bit at or above n_bits 4: instance 0"), ([0, 2], None, None)):
        w = sentinel(9, 2 * block)
        Pi, Si = [P[i] for i in order], [S[i] for i in order]
        if exc is None:
            _, _, st = api.trace_curve_msm(curve, gt.limbs(f, Pi), gt.limbs(f, Si), gt.limbs(f, start), n_bits, 2 * block, [0, block], wires=w)
            assert st.tolist() == [0, 0, NONE, 0]
        else:
            with pytest.raises(exc) as e:
                api.trace_curve_msm(curve, gt.limbs(f, Pi), gt.limbs(f, Si), gt.limbs(f, start), n_bits, 2 * block, [0, block], wires=w)
            assert text in str(e.value)
        want, _, _ = gt.trace_curve_msm(curve, Pi, Si, start, n_bits, 2 * block, [0, block])
        assert np.array_equal(w, gt.table(f, want, 9, 2 * block, base=sentinel(9, 2 * block)))
    # y = 0 in a doubling: no point of an odd-order curve has it, so the accumulator is not on the curve - the rows are computed all the same
    y0 = [(5, 0)]
    with pytest.raises(AssertionError, match="y = 0: instance 0, block row 1"):
        api.trace_curve_msm(curve, gt.limbs(f, [pts[:1]]), gt.limbs(f, [[0]]), gt.limbs(f, y0[0]), 3, 8, [0])


# ---- closed loops: judges that share nothing with the kernels ----
@pytest.mark.parametrize("curve", [0, 3])
def test_closed_loop_through_the_witness_check_and_the_group_entries(curve):
    import torch
    dev = dev_module()
    c = br.CURVES[curve]
    f, field = c.base, c.base.field_id
    n, log_n, rounds, parts, n_bits = 1 << 10, 10, 10, 2, 8
    consts, ctx = rescue_context(field, rounds)
    start = gc.start_point(curve)
    r_count, m_count = 20, 16
    r_block, m_block = gt.rescue_block_rows(rounds), gt.msm_block_rows(parts, n_bits)
    r_first = gc.back_to_back(r_count, r_block, 3)
    m_first = gc.back_to_back(m_count, m_block, 3 + r_count * r_block + 5)
    assert m_first[-1] + m_block <= n
    v = gc.values(f, 0xC105ED + curve, 4 * r_count)
    inputs = [v[4 * i:4 * i + 4] for i in range(r_count)]
    P, S = msm_inputs(curve, parts, n_bits, m_count, 0xC1 + curve)
    # Buffer prefixes everywhere (a BufferGate has no constraints), zero wires; then both entries write their blocks
    k = np.zeros((6, n, 4), dtype=np.uint64)
    k[0], k[2] = f.mont_limbs(1), f.mont_limbs(1)
    d_k, d_w = dev.to_device(k), dev.to_device(np.zeros((9, n, 4), dtype=np.uint64))
    d_in = dev.to_device(gt.limbs(f, inputs))
    _, st_r = dev.trace_rescue_permutation_dev(ctx, d_in, n, torch.tensor(r_first, dtype=torch.int32, device="cuda"), wires=d_w, constants=d_k, status=True)
    _, st_m = dev.trace_curve_msm_dev(curve, dev.to_device(gt.limbs(f, P)), dev.to_device(gt.limbs(f, S)), gt.limbs(f, start), n_bits, n,
                                      torch.tensor(m_first, dtype=torch.int32, device="cuda"), wires=d_w, constants=d_k, status=True)
    assert st_r.cpu().numpy().view(np.uint32).tolist() == st_m.cpu().numpy().view(np.uint32).tolist() == [0, 0, NONE, 0]
    zero = np.zeros(4, dtype=np.uint64)

    def report(wires):
        return api.WitnessReport(n, dev.check_witness_dev(field, log_n, d_k, wires, None, zero, zero, constants_stride=1).cpu().numpy())

    rep = report(d_w)
    assert rep.bad_rows == 0 and rep.first_row is None, (rep.bad_rows, rep.first_row, rep.first_mask)
    # one root wire and one lambda wire changed: exactly those rows, with the terms that read the wire
    w = dev.to_host(d_w).copy()
    root_row = r_first[7] + 2 * 4  # the A row of round 4: wire 5 is the root of element 1
    lam_row = next(m_first[9] + i for i in range(m_block) if i % (parts + 1) < parts and w[6, m_first[9] + i].any())  # an add row whose bit is set
    masks, kk = {}, dev.to_host(d_k)  # the constants as both entries left them
    for row, wire in ((root_row, 5), (lam_row, 8)):
        w[wire, row] = f.mont_limbs((f.from_mont(br.limbs_to_int(w[wire, row])) + 1) % f.p)
    for row in (root_row, lam_row):
        ints = lambda a: [f.from_mont(br.limbs_to_int(x)) for x in a]
        terms = br.plonk_all_constraints(f, ints(kk[:, row]), ints(w[:, row]), ints(w[:, (row + 1) % n]), ints(w[:, (row + 65) % n]), 0, 0)
        masks[row] = sum(1 << t for t, x in enumerate(terms) if x)
    assert masks == {root_row: 0b10101110, lam_row: 0b111}  # x^5 of element 1 and the four matrix rows; lambda, x4 and y4
    rm = torch.zeros(n, dtype=torch.uint8, device="cuda")
    words = dev.check_witness_dev(field, log_n, d_k, dev.to_device(w), None, zero, zero, constants_stride=1, row_masks=rm).cpu().numpy().view(np.uint32)
    got = rm.cpu().numpy()
    assert words[:3].tolist() == [2, min(masks), masks[min(masks)]]
    assert {int(i): int(got[i]) for i in np.flatnonzero(got)} == masks
    # the receiving rows are plk_rescue_permutation_dev of the same inputs
    clean = dev.to_host(d_w)
    perm = dev.to_host(dev.rescue_permutation_dev(ctx, d_in))
    assert np.array_equal(clean[:4, np.array(r_first) + 2 * rounds].transpose(1, 0, 2), perm)
    # the curve_msm results are the scalar multiples summed, plus the start multiple: scalar_mul_dev and the curve sums
    sf = c.scalar
    flat_s = np.array([sf.mont_limbs(s) for row in S for s in row] + [sf.mont_limbs(1 << (n_bits - 1))], dtype=np.uint64)
    flat_p = np.concatenate([gt.limbs(f, P).reshape(-1, 2, 4), gt.limbs(f, start).reshape(1, 2, 4)])
    prod, prod_zero = dev.scalar_mul_dev(curve, dev.to_device(flat_s), dev.to_device(flat_p))
    prod, prod_zero = dev.to_host(prod).reshape(-1, 2, 4), prod_zero.cpu().numpy()
    for i in range(m_count):
        idx = list(range(i * parts, (i + 1) * parts)) + [m_count * parts]
        xy, is_zero = api.curve_sum_affine(curve, prod[idx], prod_zero[idx])
        last = m_first[i] + m_block - 1
        assert not is_zero and np.array_equal(np.asarray(xy).reshape(2, 4), clean[:2, last]), i


def test_checked_build_runs_both_entries_clean():
    """one small case of each entry against the checked build in a fresh process: the tables as the restatement has them, every
    guard counter zero"""
    out = checked_child.run_checked('''
import numpy as np, torch
from oracle import bigint_ref as br
from plonky_amd import api, device as dev
from tests import gate_trace_cases as gc, gate_trace_ref as gt, rescue_ref as rr
dev.init(0)
f = br.FIELDS[0]
consts = rr.constants(0, 4, 2)
ctx = api.RescueContext(0, np.array(rr.constants_limbs(0, consts), dtype=np.uint64))
v = gc.values(f, 77, 12)
inputs, first = [v[0:4], v[4:8], v[8:12]], [0, 6, 11]
w, k, st = dev.to_device(np.zeros((9, 16, 4), dtype=np.uint64)), dev.to_device(np.zeros((6, 16, 4), dtype=np.uint64)), None
_, st = dev.trace_rescue_permutation_dev(ctx, dev.to_device(gt.limbs(f, inputs)), 16, torch.tensor(first, dtype=torch.int32, device="cuda"), wires=w, constants=k, status=True)
want_w, want_k, want_st = gt.trace_rescue(0, inputs, consts, 16, first)
assert st.cpu().numpy().view(np.uint32).tolist() == want_st
assert np.array_equal(dev.to_host(w), gt.table(f, want_w, 9, 16)) and np.array_equal(dev.to_host(k), gt.table(f, want_k, 6, 16))
start, pts = gc.start_point(0), gc.points(0, 5, 4)
P, S, first = [pts[:2], pts[2:]], [[5, 2], [7, 0]], [1, 12]
w2 = dev.to_device(np.zeros((9, 20, 4), dtype=np.uint64))
_, st = dev.trace_curve_msm_dev(0, dev.to_device(gt.limbs(f, P)), dev.to_device(gt.limbs(f, S)), gt.limbs(f, start), 3, 20, torch.tensor(first, dtype=torch.int32, device="cuda"), wires=w2, status=True)
want_w, _, want_st = gt.trace_curve_msm(0, P, S, start, 3, 20, first)
assert st.cpu().numpy().view(np.uint32).tolist() == want_st == [1, 0, 0xFFFFFFFF, 0]
assert np.array_equal(dev.to_host(w2), gt.table(f, want_w, 9, 20))
print("gate trace under the checked build: ok")
''')
    assert "gate trace under the checked build: ok" in out
