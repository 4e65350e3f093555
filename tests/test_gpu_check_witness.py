"""GPU tests of the witness check (include/plonky_hip_witness.h; plonk.hip k_check_rows / k_check_first / k_check_copies): the row masks,
the count, the first failing row and its eight terms against the oracle's evaluate_all_constraints row by row; a satisfied circuit with
planted faults; the copy check against numpy; the host and the device entry against each other; the refusals; the checked build.

Shapes: n = 1, 2 and 64 wrap the below index (i + 65) mod n more than once, n = 128 once, n = 2048 spans 16 workgroups of 128 lanes.
The planted rows sit at the edges of a wave (63 | 64) and of a workgroup (127 | 128)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from plonky_amd import api, lib
from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from tests import check_witness_cases as cw
from tests import checked_child
from tests import sigma_cases as sc
from tests.test_gpu_plonk import honest_tables
from tests.test_oracle_plonk import ZETA_MONT, mont

FIELDS = [br.TWEEDLEDEE_BASE, br.TWEEDLEDUM_BASE, br.BLS12_377_SCALAR, br.PALLAS_BASE, br.VESTA_BASE]
NONE = 0xFFFFFFFF
F = br.TWEEDLEDUM_BASE
ZETA = np.array(ZETA_MONT, dtype=np.uint64)


def dev_module():
    pytest.importorskip("torch")
    from plonky_amd import device as dev
    dev.init(0)
    return dev


def dev_report(dev, degree, report, first_terms=None, row_masks=None):
    return api.WitnessReport(degree, report.cpu().numpy(), None if first_terms is None else dev.to_host(first_terms),
                             None if row_masks is None else row_masks.cpu().numpy())


@functools.lru_cache(maxsize=None)
def random_case(field_id, n):
    """random tables (half the rows with the 0 / 1 selectors of one gate each, cycling the ten gates: their masks are proper subsets of
    0xFF and differ by gate) and what the oracle says of every row: (k (6, n, 4), l (9, n, 4), zeta, a, masks (n,), terms (n, 8, 4))"""
    f = next(x for x in FIELDS if x.field_id == field_id)
    k = ol.rand_field(field_id, 0xC0 + n, 6 * n).reshape(6, n, 4)
    l = ol.rand_field(field_id, 0xC1 + n, 9 * n).reshape(9, n, 4)
    zeta, a = ol.rand_field(field_id, 0xC2 + n, 2)
    one, zero = mont(f, [1])[0], mont(f, [0])[0]
    for i in range(0, n, 2):
        bits = br.PLONK_GATES[(i // 2) % len(br.PLONK_GATES)][0]
        for j, c in enumerate(bits):
            k[j, i] = one if c == "1" else zero
    terms = np.zeros((n, 8, 4), dtype=np.uint64)
    for i in range(n):
        got = ol.gate_constraints(field_id, -1, k[:, i], l[:, i], l[:, (i + 1) % n], l[:, (i + 65) % n], zeta, a)
        terms[i, :got.shape[0]] = got
    masks = (terms.any(axis=2) << np.arange(8)).sum(axis=1).astype(np.uint8)
    for arr in (k, l, terms, masks):
        arr.setflags(write=False)
    return k, l, zeta, a, masks, terms


def spread(k, seed):
    """the n-point columns inside an 8n table whose other seven eighths hold garbage"""
    n = k.shape[1]
    k8 = ol.rand_field(0, seed, 6 * 8 * n).reshape(6, 8 * n, 4)
    k8[:, ::8] = k
    return k8


def assert_rows(rep, masks, terms):
    bad = np.flatnonzero(masks)
    assert rep.bad_rows == bad.shape[0]
    if bad.shape[0]:
        first = int(bad[0])
        assert rep.first_row == first and rep.first_mask == int(masks[first])
        assert np.array_equal(rep.first_terms, terms[first])
        assert rep.message() == "%d-th gate constraints are not satisfied" % first and not rep.ok
    else:
        assert rep.first_row is None and rep.first_mask == 0 and not rep.first_terms.any() and rep.message() is None
    if rep.row_masks is not None:
        assert np.array_equal(rep.row_masks, masks)


@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
@pytest.mark.parametrize("n", [1, 2, 64, 128, 2048])
def test_rows_match_the_oracle(f, n):
    """both entries, both strides: masks byte for byte, the count, the first row, its mask, its terms word for word"""
    import torch
    dev = dev_module()
    k, l, zeta, a, masks, terms = random_case(f.field_id, n)
    assert n < 64 or len(set(masks[::2].tolist())) > 2, "the one-gate rows should give several proper subsets of 0xFF"
    k8 = spread(k, 0xD0 + n)
    log_n = api.log2_strict(n)
    for stride, table in ((1, k), (8, k8)):
        assert_rows(api.check_witness(f.field_id, n, table, l, None, zeta, a, constants_stride=stride, row_masks=True), masks, terms)
        rm, ft = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda"), torch.full((8, 4), -1, dtype=torch.int64, device="cuda")
        report = dev.check_witness_dev(f.field_id, log_n, dev.to_device(table), dev.to_device(l), None, zeta, a, constants_stride=stride, row_masks=rm,
                                       first_terms=ft)
        words = report.cpu().numpy().view(np.uint32)
        assert words[3:].tolist() == [0, NONE, 0, 0, 0]
        assert_rows(dev_report(dev, n, report, ft, rm), masks, terms)
    # without the optional outputs: the same report
    lean = api.check_witness(f.field_id, n, k, l, None, zeta, a)
    assert lean.row_masks is None and lean.bad_rows == np.count_nonzero(masks)
    bad = np.flatnonzero(masks)
    words = dev.check_witness_dev(f.field_id, log_n, dev.to_device(k), dev.to_device(l), None, zeta, a, constants_stride=1).cpu().numpy().view(np.uint32)
    assert words[:3].tolist() == ([bad.shape[0], int(bad[0]), int(masks[bad[0]])] if bad.shape[0] else [0, NONE, 0])


@functools.lru_cache(maxsize=None)
def honest(log_degree):
    consts, wires = honest_tables(F, 1 << min(log_degree, 12), 4242 + log_degree)
    reps = 1 << max(0, log_degree - 12)  # every row is satisfied on its own wires: a tiling of a satisfied table is one
    consts, wires = np.tile(consts, (1, reps, 1)), np.tile(wires, (1, reps, 1))
    consts.setflags(write=False)
    wires.setflags(write=False)
    return consts, wires


def planted(n, count):
    """row 0, row n - 1, the last lane of a wave, the first lane of the next wave and of the next workgroup, then seeded rows"""
    if count == 1:
        return [0]
    if count == 2:
        return [63, n - 1]
    rows = sorted({r for r in (0, n - 1, 63, 64, 127, 128) if r < n})
    rng = np.random.default_rng(n + count)
    while len(rows) < count:
        r = int(rng.integers(0, n))
        if r not in rows:
            rows.append(r)
    return sorted(rows)


@pytest.mark.parametrize("log_degree", [7, 12])
def test_satisfied_circuit_and_planted_faults(log_degree):
    n = 1 << log_degree
    consts, wires = honest(log_degree)
    a0 = mont(F, [0])[0]
    identity = np.arange(6 * n, dtype=np.uint32)
    rep = api.check_witness(F.field_id, n, consts, wires, identity, ZETA, a0, row_masks=True)
    assert rep.ok and rep.first_row is None and rep.first_copy is None and not rep.row_masks.any() and rep.message() is None
    assert (rep.bad_rows, rep.first_mask, rep.bad_copies, rep.sigma_out_of_range) == (0, 0, 0, 0) and not rep.first_terms.any()
    for count in (1, 2, 65):
        rows = planted(n, count)
        assert len(rows) == count and (count < 65 or {0, n - 1, 63, 64, 127 % n}.issubset(rows))
        w = wires.copy()
        for r in rows:
            cw.break_row(w, r, mont(F, [12345 + r])[0])
        rep = api.check_witness(F.field_id, n, consts, w, identity, ZETA, a0, row_masks=True)
        assert np.flatnonzero(rep.row_masks).tolist() == rows and rep.bad_rows == count and rep.first_row == rows[0]
        assert rep.first_mask == int(rep.row_masks[rows[0]]) and rep.bad_copies == 0 and not rep.ok
        i = rows[0]
        exp = ol.gate_constraints(F.field_id, -1, consts[:, i], w[:, i], w[:, (i + 1) % n], w[:, (i + 65) % n], ZETA, a0)
        assert np.array_equal(rep.first_terms, exp)
    # a wire that only the row to its left reads: row 5 becomes a PublicInputGate (101001: its wires 6..8 against wires 0..2 of row 6),
    # row 6 is a ConstantGate and reads its own wire 0 alone
    k, w = consts.copy(), wires.copy()
    one, zero = mont(F, [1])[0], mont(F, [0])[0]
    for j, c in enumerate("101001"):
        k[j, 5] = one if c == "1" else zero
    w[6:9, 5] = w[0:3, 6]
    assert api.check_witness(F.field_id, n, k, w, None, ZETA, a0).ok
    w[1, 6] = mont(F, [777])[0]
    rep = api.check_witness(F.field_id, n, k, w, None, ZETA, a0, row_masks=True)
    assert (rep.bad_rows, rep.first_row, rep.first_mask) == (1, 5, 0b010) and np.flatnonzero(rep.row_masks).tolist() == [5]


def test_planted_faults_at_full_grid_size():
    """2^16 rows, 512 workgroups: the planted rows only, no oracle loop"""
    import torch
    dev = dev_module()
    log_degree, n = 16, 1 << 16
    consts, wires = honest(log_degree)
    rows = [63, 64, 127, 128, 4095, 4096, 40000, n - 1]
    w = wires.copy()
    for r in rows:
        cw.break_row(w, r, mont(F, [999 + r])[0], period=1 << 12)
    rm = torch.zeros(n, dtype=torch.uint8, device="cuda")
    report = dev.check_witness_dev(F.field_id, log_degree, dev.to_device(consts), dev.to_device(w), None, ZETA, mont(F, [0])[0], constants_stride=1, row_masks=rm)
    rep = dev_report(dev, n, report, None, rm)
    assert np.flatnonzero(rep.row_masks).tolist() == rows and (rep.bad_rows, rep.first_row) == (len(rows), 63)
    assert rep.first_mask == int(rep.row_masks[63])


def partitioned_witness(n, seed):
    """partitions through api.TargetPartitions (a partition of 3 in one column, one across two columns, wire 0 and wire 6n - 1 in
    company, seeded merges), their sigma from the device, and wires whose values are equal within every partition"""
    dev = dev_module()
    w = lambda g, i: ("wire", g, i)
    ops = [(w(0, 0), w(1, 0)), (w(2, 0), w(0, 0)), (w(3, 1), w(5, 4)), (w(n - 1, 5), w(4, 2))] + sc.merge_sequence(n, seed, n_virtual=4, n_merges=2 * n, cap=5)
    wp = sc.build_partitions(api.TargetPartitions, n, ops, 4).to_wire_partitions()
    members, offsets = wp.to_csr(n)
    k_is = ol.rand_field(F.field_id, 5, 6)
    sigma, _ = dev.sigma_dev(F.field_id, api.log2_strict(n), _i32(members), _i32(offsets), k_is)
    label = np.array([[wp.indices[(g, i)] for g in range(n)] for i in range(9)])
    values = ol.rand_field(F.field_id, seed + 1, len(wp.partitions))
    return wp, sigma, values[label]  # (9, n, 4)


def _i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to("cuda")


def numpy_copies(wires, sigma, n):
    flat = wires.reshape(9 * n, 4)
    s = sigma.astype(np.int64)
    inside = s < 6 * n
    differs = np.zeros(6 * n, dtype=bool)
    differs[inside] = (flat[:6 * n][inside] != flat[s[inside]]).any(axis=1)
    bad = np.flatnonzero(differs)
    return bad.shape[0], (int(bad[0]) if bad.shape[0] else None), int((~inside).sum())


def test_copy_check_against_numpy():
    dev = dev_module()
    n, log_n = 256, 8
    wp, sigma_t, wires = partitioned_witness(n, 0xC0B1)
    sigma = sigma_t.cpu().numpy().view(np.uint32)
    assert len(wp.partitions[wp.indices[(0, 0)]]) >= 3 and wp.indices[(3, 1)] == wp.indices[(5, 4)] and wp.indices[(n - 1, 5)] == wp.indices[(4, 2)]
    consts = ol.rand_field(F.field_id, 3, 6 * n).reshape(6, n, 4)
    a0 = mont(F, [0])[0]

    def copies(w, s_t):
        report = dev.check_witness_dev(F.field_id, log_n, dev.to_device(consts), dev.to_device(w), s_t, ZETA, a0, constants_stride=1)
        rep = dev_report(dev, n, report)
        first = None if rep.first_copy is None else rep.first_copy[0] * n + rep.first_copy[1]
        return rep.bad_copies, first, rep.sigma_out_of_range

    assert copies(wires, sigma_t) == numpy_copies(wires, sigma, n) == (0, None, 0)
    odd = mont(F, [31337])[0]
    for inp, gate in ((0, 1), (4, 5), (0, 0), (5, n - 1)):  # a member of the partition of 3, the second column of a pair, wire 0, wire 6n - 1
        w = wires.copy()
        w[inp, gate] = odd
        got = copies(w, sigma_t)
        assert got == numpy_copies(w, sigma, n) and got[0] >= 1 and got[2] == 0, (inp, gate, got)
    # the host entry sees the same
    w = wires.copy()
    w[0, 1] = odd
    rep = api.check_witness(F.field_id, n, consts, w, sigma, ZETA, a0)
    exp = numpy_copies(w, sigma, n)
    assert (rep.bad_copies, rep.first_copy, rep.sigma_out_of_range) == (exp[0], (exp[1] // n, exp[1] % n), 0)
    # entries that are not below 6n are counted and not followed: 6n, 0xFFFFFFFF and 9n - 1 (inside the wire table, outside the routed rows)
    s = sigma.copy()
    s[[7, n + 3, 6 * n - 2]] = [6 * n, 0xFFFFFFFF, 9 * n - 1]
    got = copies(w, _i32(s))
    assert got == numpy_copies(w, s, n) and got[2] == 3
    # no sigma: words 3..5 stay as initialised
    report = dev.check_witness_dev(F.field_id, log_n, dev.to_device(consts), dev.to_device(w), None, ZETA, a0, constants_stride=1)
    assert report.cpu().numpy().view(np.uint32)[3:].tolist() == [0, NONE, 0, 0, 0]


def test_circuit_key_tables_go_in_unchanged():
    """circuit_key_dev's own constants_8n (stride 8) and sigma at 2^10: satisfied, then one fault and one broken copy"""
    import torch
    dev = dev_module()
    log_degree, n = 10, 1 << 10
    consts, wires = honest(log_degree)
    pairs = [[w, w + 1] for w in range(0, 6 * n, 2)]  # neighbours in a column share a value below
    members, offsets = sc.csr(pairs + [[w] for w in range(6 * n, 9 * n)])
    k_is = ol.rand_field(F.field_id, 5, 6)
    assert api.CURVE_SCALAR_FIELD[br.TWEEDLEDEE.curve_id] == F.field_id
    key = dev.circuit_key_dev(br.TWEEDLEDEE.curve_id, log_degree, dev.to_device(np.ascontiguousarray(consts.transpose(1, 0, 2))), _i32(members),
                              _i32(offsets), k_is)
    a0 = mont(F, [0])[0]
    d_wires = dev.to_device(wires)
    rep = dev_report(dev, n, dev.check_witness_dev(F.field_id, log_degree, key.constants_8n, d_wires, None, ZETA, a0))
    assert rep.bad_rows == 0 and rep.first_row is None
    # the honest wires are random, so the pairs differ: every routed wire mismatches, the first is wire 0
    rep = dev_report(dev, n, dev.check_witness_dev(F.field_id, log_degree, key.constants_8n, d_wires, key.sigma, ZETA, a0))
    exp = numpy_copies(wires, key.sigma.cpu().numpy().view(np.uint32), n)
    assert (rep.bad_rows, rep.bad_copies, rep.first_copy, rep.sigma_out_of_range) == (0, exp[0], (0, 0), 0) and exp[1] == 0
    w = wires.copy()
    cw.break_row(w, 700, mont(F, [4])[0])
    ft = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    rep = dev_report(dev, n, dev.check_witness_dev(F.field_id, log_degree, key.constants_8n, dev.to_device(w), None, ZETA, a0, first_terms=ft), ft)
    exp = ol.gate_constraints(F.field_id, -1, consts[:, 700], w[:, 700], w[:, 701], w[:, 765], ZETA, a0)
    assert (rep.bad_rows, rep.first_row) == (1, 700) and np.array_equal(rep.first_terms, exp)
    assert rep.message() == "700-th gate constraints are not satisfied"


def test_refusals_with_a_device_present():
    """every refusal comes before anything is launched: the same codes and texts as without a device"""
    dev_module()
    results = cw.refusal_results(lib.load())
    assert len(results) == 2 * len(cw.REFUSALS)
    for (entry, name, rc, text), (_, _, starts) in zip(results, cw.REFUSALS * 2):
        assert rc == lib.PLK_ERR_INVALID_ARG and text.startswith(starts), (entry, name, rc, text)


CHECKED_BODY = '''
import numpy as np
import torch
from plonky_amd import api, device as dev
from oracle import bigint_ref as br
from tests import check_witness_cases as cw
from tests.test_gpu_plonk import honest_tables
from tests.test_oracle_plonk import ZETA_MONT, mont
dev.init(0)
f, n = br.TWEEDLEDUM_BASE, 128
consts, wires = honest_tables(f, n, 4249)
zeta, a0 = np.array(ZETA_MONT, dtype=np.uint64), mont(f, [0])[0]
sigma = np.arange(6 * n, dtype=np.uint32)
assert api.check_witness(f.field_id, n, consts, wires, sigma, zeta, a0).ok
cw.break_row(wires, 64, mont(f, [5])[0])
wires[2, 9] = mont(f, [6])[0]
sigma[2 * n + 9], sigma[2 * n + 10] = 2 * n + 10, 2 * n + 9
rep = api.check_witness(f.field_id, n, consts, wires, sigma, zeta, a0, row_masks=True)
rm = torch.zeros(n, dtype=torch.uint8, device="cuda")
words = dev.check_witness_dev(f.field_id, 7, dev.to_device(consts), dev.to_device(wires), torch.from_numpy(sigma.view(np.int32)).cuda(), zeta, a0,
                              constants_stride=1, row_masks=rm).cpu().numpy().view(np.uint32).tolist()
assert np.array_equal(rm.cpu().numpy(), rep.row_masks)
assert words[1] == rep.first_row and words[3] == rep.bad_copies == 2 and words[4] == 2 * n + 9 and rep.first_copy == (2, 9)
print("WITNESS", words)
'''


def test_checked_build_runs_the_same_set():
    out = checked_child.run_checked(CHECKED_BODY)
    assert "WITNESS" in out
