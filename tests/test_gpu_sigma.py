"""GPU tests of the copy-constraint permutation on the device (plk_plonk_sigma[_dev], sigma.hip): sigma against the restatement of
partition.rs (tests/partition_ref.py) and the numpy neighbour rule, the values against Python integers and against ident[sigma]
(ident: the device NTT of k_j X, as tests/test_gpu_permutation.honest_copy_cycles builds it), the status words, the chain into the
grand product Z, device.circuit_key_dev against the same steps one by one, and the host-pointer form.  No id out of range goes to
the GPU: that case is replayed on the host (tests/test_sigma_host_replay.py)."""
import functools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from plonky_amd import api
from tests import partition_ref as pref
from tests import sigma_cases as sc
from tests.test_oracle_plonk import mont, unmont

FIELDS = [br.TWEEDLEDEE_BASE, br.TWEEDLEDUM_BASE, br.BLS12_377_SCALAR, br.PALLAS_BASE, br.VESTA_BASE]
by_field = pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)


def shifts(f, seed=0x5161):
    rng = random.Random(seed + f.field_id)
    k = [rng.randrange(1, f.p) for _ in range(6)]
    return k, mont(f, k)


def words(t):
    return t.cpu().numpy().view(np.uint32)


def to_dev32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def run(f, log_n, members, offsets, km, want_sigma=True):
    """(sigma (6n,) uint32, values (6n, 4) uint64, status words) of the device form"""
    from plonky_amd import device as dev
    dev.init(0)
    sigma, vals, st = dev.sigma_dev(f.field_id, log_n, to_dev32(members), to_dev32(offsets), km, want_sigma=want_sigma, status=True)
    return (words(sigma) if want_sigma else None), dev.to_host(vals).reshape(-1, 4), words(st).tolist()


def ident_table(f, log_n, km):
    """k_j g^r, (6n, 4): the device NTT of the polynomials k_j X"""
    from plonky_amd import device as dev
    n = 1 << log_n
    coeffs = np.zeros((6, n, 4), dtype=np.uint64)
    coeffs[:, 1] = km
    return dev.to_host(dev.ntt_dev(f.field_id, dev.to_device(coeffs))).reshape(6 * n, 4)


def check_full(f, log_n, members, offsets, exp_sigma=None, samples=None):
    """sigma against exp_sigma (the numpy rule when not given), the values against ident[sigma] in full (n >= 2) and against Python
    integers (everywhere, or at `samples` seeded positions)"""
    n = 1 << log_n
    k, km = shifts(f)
    sigma, vals, status = run(f, log_n, members, offsets, km)
    assert status == [0, 0, 0]
    exp_sigma = sc.neighbour_rule(members, offsets, n) if exp_sigma is None else np.asarray(exp_sigma, dtype=np.uint32)
    assert np.array_equal(sigma, exp_sigma)
    if n >= 2:
        assert np.array_equal(vals, ident_table(f, log_n, km)[sigma.astype(np.int64)])
    pos = np.arange(6 * n) if samples is None else np.sort(np.random.default_rng(0x5A3 + log_n).choice(6 * n, size=samples, replace=False))
    g = f.primitive_root_of_unity(log_n)
    exp = [k[int(x) // n] * pow(g, int(x) % n, f.p) % f.p for x in exp_sigma[pos]]
    assert unmont(f, vals[pos]) == exp
    # the same values without sigma: the form a prover that only wants S_sigma calls
    _, vals2, status2 = run(f, log_n, members, offsets, km, want_sigma=False)
    assert status2 == [0, 0, 0] and np.array_equal(vals2, vals)
    return sigma, vals


def ref_sigma(members, offsets, n):
    """to_sigma of the restated reference on the listed partitions (non-routed wires a listing leaves out are only counted there)"""
    wp = pref.csr_to_wire_partitions(members, offsets, n)
    for g in range(n):
        for i in range(pref.NUM_WIRES):
            wp.indices.setdefault((g, i), -1)
    wp.assert_valid()
    return wp.to_sigma()


@by_field
@pytest.mark.parametrize("log_n", [0, 1, 2])
def test_degenerate_sizes(f, log_n):
    n = 1 << log_n
    for listed in (True, False):
        sigma, vals = check_full(f, log_n, *sc.singletons(n, listed), exp_sigma=np.arange(6 * n))
    k, _ = shifts(f)
    g = f.primitive_root_of_unity(log_n)
    assert unmont(f, vals) == [k[j] * pow(g, r, f.p) % f.p for j in range(6) for r in range(n)]


@by_field
@pytest.mark.parametrize("log_n", [2, 8])
def test_one_cycle_through_everything(f, log_n):
    n = 1 << log_n
    members, offsets = sc.one_cycle(n, 0xC1C + log_n)
    sigma, _ = check_full(f, log_n, members, offsets, exp_sigma=ref_sigma(members, offsets, n))
    assert sigma[members[-1]] == members[0]  # the wrap from the last slot to offsets[q]
    assert np.any(sigma // n != np.arange(6 * n) // n)  # neighbours cross columns
    seen, w = 0, 0
    while True:  # one cycle of length 6n
        w, seen = int(sigma[w]), seen + 1
        if w == 0:
            break
    assert seen == 6 * n


@by_field
def test_listing_variants_give_one_sigma(f):
    n = 16
    variants = sc.listing_variants(n, 0x715)
    assert len(variants) >= 6
    exp = ref_sigma(*variants["pairs only"], n)
    for name, (members, offsets) in variants.items():
        check_full(f, 4, members, offsets, exp_sigma=exp)


@by_field
def test_workgroup_seams(f):
    n = 1 << 10
    members, offsets = sc.seams(n, 0x5EA)
    sizes = np.diff(offsets.astype(np.int64)).tolist()
    assert sizes[:5] == list(sc.SEAM_SIZES) and sum(sizes) == 6 * n
    begins, ends = offsets[:-1].astype(np.int64), offsets[1:].astype(np.int64)
    assert {int(e) % 256 for e in ends} >= {255, 0}  # the wrapping slot is the last but one or the last lane of a 256-slot workgroup
    assert np.any(begins // 256 != (ends - 1) // 256) and np.any((ends - 1) // 256 - begins // 256 >= 4)  # wraps into other workgroups
    check_full(f, 10, members, offsets, exp_sigma=ref_sigma(members, offsets, n))


@functools.lru_cache(maxsize=None)
def merged(log_n, cap):
    """(members, offsets) through api.TargetPartitions for a seeded merge sequence with virtual targets and stale lists"""
    n = 1 << log_n
    n_virtual = n // 4
    ops = sc.merge_sequence(n, 0xAB0 + log_n, n_virtual=n_virtual, n_merges=3 * n, cap=cap)
    tp = sc.build_partitions(api.TargetPartitions, n, ops, n_virtual)
    pointed = set(tp.indices.values())
    assert any(q not in pointed and len(part) > 1 for q, part in enumerate(tp.partitions)), "no stale list"
    members, offsets = tp.to_wire_partitions().to_csr(n)
    if cap is not None:
        assert np.diff(offsets.astype(np.int64)).max() <= cap
    ref = None
    if log_n <= 10:
        ref = sc.build_partitions(pref.TargetPartitionsRef, n, ops, n_virtual).to_wire_partitions().to_sigma()
    return members, offsets, ref


@by_field
def test_random_merges_2p10(f):
    members, offsets, ref = merged(10, None)
    assert np.diff(offsets.astype(np.int64)).max() > 2
    check_full(f, 10, members, offsets, exp_sigma=ref, samples=4096)


@by_field
def test_random_merges_2p16(f):
    members, offsets, _ = merged(16, 32)
    check_full(f, 16, members, offsets, samples=4096)


def test_skew_2p20():
    """one partition of 2^19 members among singletons: the numpy rule and ident[sigma]"""
    f, log_n = br.TWEEDLEDUM_BASE, 20
    n = 1 << log_n
    members, offsets = sc.skew(n, 0x5CE)
    assert np.diff(offsets.astype(np.int64)).max() == n // 2 and members.shape[0] == 6 * n
    k, km = shifts(f)
    sigma, vals, status = run(f, log_n, members, offsets, km)
    assert status == [0, 0, 0]
    assert np.array_equal(sigma, sc.neighbour_rule(members, offsets, n))
    assert np.array_equal(vals, ident_table(f, log_n, km)[sigma.astype(np.int64)])


@by_field
def test_status_words(f):
    n, log_n = 16, 4
    _, km = shifts(f)
    cases = sc.bad_cases(n, 0x715)
    assert set(cases) == {"one wire listed twice", "one wire left out", "a non-routed wire in a pair", "valid"}
    texts = {"one wire listed twice": "no entry found for key", "one wire left out": "no entry found for key",
             "a non-routed wire in a pair": "Non-routed wires should not be in a partition containing other wires"}
    for name, (members, offsets, exp) in cases.items():
        assert int(members.max()) < 9 * n  # no id out of range on the GPU
        assert pref.status_words_ref(members, offsets, n) == exp
        for want_sigma in (True, False):
            assert run(f, log_n, members, offsets, km, want_sigma)[2] == exp, (name, want_sigma)
        if name == "valid":
            sigma, vals = api.wire_partitions_to_sigma(f.field_id, n, members, offsets, km)
            assert np.array_equal(sigma, sc.neighbour_rule(members, offsets, n))
        else:
            with pytest.raises(AssertionError, match=texts[name]):
                api.wire_partitions_to_sigma(f.field_id, n, members, offsets, km)


def test_chain_into_the_grand_product():
    """pooled wires -> api.TargetPartitions (cells of equal value merged in a seeded order) -> sigma_dev -> Z closes the cycle; with the
    members of two partitions of different values exchanged it does not"""
    from plonky_amd import device as dev
    from tests.test_gpu_permutation import pooled_wires
    dev.init(0)
    f, log_n = br.TWEEDLEDUM_BASE, 10
    n = 1 << log_n
    rng = random.Random(0xC4A1)
    k, km = shifts(f)
    bm, gm = mont(f, [rng.randrange(f.p)])[0], mont(f, [rng.randrange(f.p)])[0]
    w, idx = pooled_wires(f, log_n, 0xC0DE + log_n)
    cells = {}
    for j in range(6):
        for r in range(n):
            cells.setdefault(int(idx[j, r]), []).append(("wire", r, j))
    links = []
    for group in cells.values():
        rng.shuffle(group)
        links += list(zip(group[:-1], group[1:]))
    rng.shuffle(links)
    tp = sc.build_partitions(api.TargetPartitions, n, links, 0)
    members, offsets = tp.to_wire_partitions().to_csr(n)
    dw = dev.to_device(w)

    def z_status(m):
        _, vals, st = dev.sigma_dev(f.field_id, log_n, to_dev32(m), to_dev32(offsets), km, status=True)
        assert words(st).tolist() == [0, 0, 0]
        _, zst = dev.permutation_polynomial_dev(f.field_id, log_n, dw, vals, km, bm, gm, sigma_stride=1, status=True)
        return zst.cpu().tolist()

    assert z_status(members) == [0, 1]
    sizes = np.diff(offsets.astype(np.int64))
    big = [q for q in range(sizes.shape[0]) if sizes[q] > 1]
    qa = big[0]
    value = lambda m: int(idx[int(m) // n, int(m) % n])
    qb = next(q for q in big[1:] if value(members[offsets[q]]) != value(members[offsets[qa]]))
    swapped = members.copy()
    swapped[offsets[qa]], swapped[offsets[qb]] = members[offsets[qb]], members[offsets[qa]]
    assert z_status(swapped)[1] == 0


@pytest.mark.parametrize("c", [br.TWEEDLEDEE, br.PALLAS], ids=lambda c: c.name)
def test_circuit_key(c):
    """every field of circuit_key_dev bit-equal to the same steps one by one through the existing entry points, from sigma values built
    on the host; c_s_sigmas also through the host path of the commitments"""
    import torch
    from plonky_amd import device as dev
    from oracle import oracle_lib as ol
    dev.init(0)
    f, log_n = c.scalar, 10
    n = 1 << log_n
    _, km = shifts(f)
    members, offsets, ref = merged(10, None)
    gate_constants = ol.rand_field(f.field_id, 0xC0157 + c.curve_id, n * 6).reshape(n, 6, 4)
    key = dev.circuit_key_dev(c.curve_id, log_n, dev.to_device(gate_constants), to_dev32(members), to_dev32(offsets), km)
    same = lambda t, a: np.array_equal(dev.to_host(t).reshape(a.shape), a)
    # the steps one by one
    gens = dev.hash_to_curve_dev(c.curve_id, n + 2)
    assert torch.equal(key.pedersen_g, gens[:n]) and torch.equal(key.pedersen_h, gens[n]) and torch.equal(key.u, gens[n + 1])
    pre = dev.msm_precompute_dev(c.curve_id, gens[: n + 1].contiguous(), w=11)
    assert len(key.msm_precomputation) == n + 1 and key.msm_precomputation.w == 11
    blind = torch.zeros((6, 1, 4), dtype=torch.int64, device="cuda")
    wire_constants = np.ascontiguousarray(gate_constants.transpose(1, 0, 2))
    polys = dev.ntt_dev(f.field_id, dev.to_device(wire_constants), inverse=True)
    assert torch.equal(key.constant_polynomials, polys)
    assert torch.equal(key.constants_8n, dev.ntt_padded_dev(f.field_id, polys, log_n + 3))
    xy, z = dev.msm_execute_dev(pre, torch.cat([polys, blind], dim=1).contiguous())
    assert torch.equal(key.c_constants[0], xy) and torch.equal(key.c_constants[1], z)
    sigma = np.array(ref, dtype=np.int64)  # to_sigma of the restated reference
    assert np.array_equal(words(key.sigma), sigma.astype(np.uint32))
    host_values = ident_table(f, log_n, km)[sigma].reshape(6, n, 4)
    s_polys = dev.ntt_dev(f.field_id, dev.to_device(host_values), inverse=True)
    assert torch.equal(key.s_sigma_polynomials, s_polys)
    assert torch.equal(key.s_sigma_values_8n, dev.ntt_padded_dev(f.field_id, s_polys, log_n + 3))
    xy, z = dev.msm_execute_dev(pre, torch.cat([s_polys, blind], dim=1).contiguous())
    assert torch.equal(key.c_s_sigmas[0], xy) and torch.equal(key.c_s_sigmas[1], z)
    # the host path of the commitments (poly_commit.rs:51-66, blinding off)
    g_host = dev.to_host(gens)
    hpre = api.commitment_precompute(c.curve_id, g_host[:n], g_host[n:n + 1], 11)
    pts, zeros = api.coeffs_vec_to_commitments(hpre, dev.to_host(s_polys), np.zeros((6, 4), dtype=np.uint64))
    assert same(key.c_s_sigmas[0], pts) and np.array_equal(key.c_s_sigmas[1].cpu().numpy(), zeros)
    assert same(key.s_sigma_polynomials, api.values_to_polynomials(api.sigma_polynomials(f.field_id, sigma, n, km), api.fft_precompute(f.field_id, n)))


def test_pointer_forms_agree():
    f, log_n = br.PALLAS_BASE, 12
    n = 1 << log_n
    _, km = shifts(f)
    ops = sc.merge_sequence(n, 0xF0A, n_virtual=64, n_merges=2 * n, cap=64)
    members, offsets = sc.build_partitions(api.TargetPartitions, n, ops, 64).to_wire_partitions().to_csr(n)
    sigma, vals, status = run(f, log_n, members, offsets, km)
    assert status == [0, 0, 0]
    h_sigma, h_vals = api.wire_partitions_to_sigma(f.field_id, n, members, offsets, km)
    assert np.array_equal(h_sigma, sigma) and np.array_equal(h_vals.reshape(-1, 4), vals)
    assert np.array_equal(api.wire_partitions_to_sigma(f.field_id, n, members, offsets, km, want_values=False), sigma)
