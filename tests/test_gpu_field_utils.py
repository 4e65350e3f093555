"""GPU tests of the small utility kernels everything else calls: Field::square_root (fe_sqrt.cuh, through the "sqrt" / "sqrt_tabled" ops
of plk_field_op), the batch inversion and the batch normalisation (k_batch_inverse, k_batch_to_affine), the scalar side of an IPA round
(k_inner_product, k_fold_slices) and the byte encodings (serial.hip).  Everything is exact field arithmetic: every comparison is bit for
bit, against Python integers, and against the oracle where it decides which of two roots is returned.

Stored words are Montgomery form (value * R mod p, R = 2^(64 L)).  A Montgomery product of stored words a, b is a b R^-1 mod p, so the
references of the inner product and of the fold work on the stored words directly: one multiplication by R^-1 per result.

Kernel geometry the sizes are named after (fieldops.hip, serial.hip): the two batch kernels give every lane a chain of BATCH_PER_LANE = 8
elements strided by the grid, slot k of lane t is index t + k * lanes with lanes = 128 * ceil(ceil(n / 8) / 128), so up to n = 128 every
lane holds ONE real element and the prefix products and the back substitution only do work above that; the inner product runs at most
1024 workgroups of 256 lanes, so a lane takes a second grid-stride trip only above 262144 elements; the field encodings run workgroups
of 128 lanes, the point decompression of 64.
"""
import functools
import itertools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from plonky_amd import api, synth
from tests import sqrt_cases as sc

FIELDS = sc.FIELDS
CURVES = [br.CURVES[i] for i in sorted(br.CURVES)]
BATCH_PER_LANE, BATCH_BLOCK = 8, 128
N_BATCH = [1, 7, 8, 9, 127, 128, 129, 1023, 1024, 1025, 2049]
N_DEV = [9, 129, 1025, 2049]
IP_N = [0, 1, 255, 256, 257, 511, 65537]
IP_SECOND_TRIP = 1024 * 256 + 257  # the smallest size at which only SOME lanes take a second grid-stride trip
FOLD_N = [1, 255, 256, 257, 4097]
name = lambda x: x.name  # noqa: E731


def _gpu():
    import torch
    from plonky_amd import device as dev, lib
    return torch, dev, lib


# ---- stored words <-> Python integers ----
def words_to_ints(arr):
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    step = 8 * a.shape[-1]
    b = a.tobytes()
    return [int.from_bytes(b[i:i + step], "little") for i in range(0, len(b), step)]


def ints_to_words(vals, L):
    if not len(vals):
        return np.zeros((0, L), dtype=np.uint64)
    return np.frombuffer(b"".join(int(v).to_bytes(8 * L, "little") for v in vals), dtype=np.uint64).reshape(len(vals), L).copy()


# =============================================================================================
# Field::square_root at every 2-adic depth (tests/sqrt_cases.py)
# =============================================================================================
@functools.lru_cache(maxsize=None)
def sqrt_table(fid):
    f = br.FIELDS[fid]
    none = (1 << (64 * f.n_limbs)) - 1  # all words 0xFFFFFFFF
    cases = sc.build_cases(f)
    want = []
    for label, a, ks in cases:
        root, walked = sc.restated_sqrt(f, a)
        assert (root is None) == (ks is None) and (ks is None or walked == ks), label
        want.append(none if root is None else f.to_mont(root))
    return cases, ints_to_words([f.to_mont(a) for _, a, _ in cases], f.n_limbs), want, none


@pytest.mark.parametrize("op", ["sqrt", "sqrt_tabled"])
@pytest.mark.parametrize("f", FIELDS, ids=name)
def test_square_root_at_every_depth(f, op):
    """fe_sqrt / fe_sqrt_tabled on the whole case table in one call: a single step at every depth k = 1 .. A - 1, descending runs from
    every depth (the longest walks every depth once), b = 1 at entry, a = 0, odd exponents (the k >= v exit).  The root is the
    restatement's, limb for limb - the same one of the two roots - and the non-residue marker sits exactly where it was intended."""
    cases, x, want, none = sqrt_table(f.field_id)
    got = words_to_ints(api.field_op(f.field_id, op, x))
    assert len(got) == len(cases)
    for (label, _, ks), g, w in zip(cases, got, want):
        assert (g == none) == (ks is None), (label, ks)
        assert g == w, (label, ks)


# =============================================================================================
# Field::batch_multiplicative_inverse[_opt]
# =============================================================================================
def batch_lanes(n):
    return BATCH_BLOCK * -(-(-(-n // BATCH_PER_LANE)) // BATCH_BLOCK)


def chain(n, t):
    """the indices lane t holds, first slot first"""
    lanes = batch_lanes(n)
    return [t + k * lanes for k in range(BATCH_PER_LANE) if t + k * lanes < n]


def test_the_geometry_these_tests_assume():
    assert [batch_lanes(n) for n in N_BATCH] == [128] * 9 + [256, 384]
    assert [len(chain(n, 0)) for n in N_BATCH] == [1] * 6 + [2, 8, 8, 5, 6]
    assert chain(1025, 0)[-1] == 1024 and chain(2049, 3) == [3, 387, 771, 1155, 1539, 1923]
    assert sorted(i for t in range(batch_lanes(2049)) for i in chain(2049, t)) == list(range(2049))


@functools.lru_cache(maxsize=None)
def inverse_inputs(fid, n):
    """stored words: seeded values with 1, 2, p - 1 and (p + 1) / 2 at index 0, at n - 1 and either side of every chain boundary; and
    their inverses (x R -> x^-1 R = R^2 / (x R))"""
    f = br.FIELDS[fid]
    p, lanes = f.p, batch_lanes(n)
    vals = [v or 1 for v in words_to_ints(synth.rand_field(fid, 0xBA7C0000 + n, n))]
    spots = sorted({0, n - 1} | {i for k in range(1, BATCH_PER_LANE + 1) for i in (k * lanes - 1, k * lanes) if i < n})
    for j, i in enumerate(spots):
        vals[i] = f.to_mont((1, 2, p - 1, (p + 1) // 2)[j % 4])
    return vals, [pow(v, -1, p) * f.R2 % p for v in vals]


def zero_patterns(n):
    ch = chain(n, min(3, n - 1))
    return {"one_lanes_whole_chain": ch, "first_slot": ch[:1], "last_real_slot": ch[-1:], "index_0": [0], "index_last": [n - 1],
            "every_element": list(range(n))}


@pytest.mark.parametrize("f", FIELDS, ids=name)
def test_batch_inverse_values_and_zero_patterns(f):
    _, _, lib = _gpu()
    fid, L = f.field_id, f.n_limbs
    for n in N_BATCH:
        vals, inv = inverse_inputs(fid, n)
        x = ints_to_words(vals, L)
        assert words_to_ints(api.batch_multiplicative_inverse(fid, x)) == inv, n
        got, none = api.batch_multiplicative_inverse_opt(fid, x)
        assert words_to_ints(got) == inv and not none.any(), n
        for pattern, zs in zero_patterns(n).items():
            xz = x.copy()
            xz[zs] = 0
            flags = np.zeros(n, dtype=np.uint8)
            flags[zs] = 1
            want = list(inv)
            for i in zs:
                want[i] = 0
            got, none = api.batch_multiplicative_inverse_opt(fid, xz)
            assert np.array_equal(none, flags), (n, pattern)  # the flags are exact
            assert words_to_ints(got) == want, (n, pattern)  # flagged outputs are zero, no other output is disturbed
            with pytest.raises(AssertionError, match="No inverse"):
                api.batch_multiplicative_inverse(fid, xz)
            text = lib.load().plk_last_error().decode()
            assert text.startswith("No inverse: %d of the %d elements are zero" % (len(zs), n)), (n, pattern, text)


@pytest.mark.parametrize("f", FIELDS, ids=name)
def test_batch_inverse_dev_out_of_place_in_place_and_without_flags(f):
    """plk_field_batch_inverse_dev itself on device buffers: out of place, with d_is_none == NULL, and in place (d_out == d_x, which the
    header allows): the same words all three times."""
    torch, dev, lib = _gpu()
    L = lib.load()
    fid = f.field_id
    for n in N_DEV:
        vals, inv = inverse_inputs(fid, n)
        zs = sorted(set(zero_patterns(n)["one_lanes_whole_chain"] + [n - 1]))
        x = ints_to_words(vals, f.n_limbs)
        x[zs] = 0
        want = list(inv)
        for i in zs:
            want[i] = 0
        flags = np.zeros(n, dtype=np.uint8)
        flags[zs] = 1
        dx = dev.to_device(x)
        keep = dx.clone()
        out = torch.full_like(dx, 0x5A5A)
        none = torch.full((n,), 7, dtype=torch.uint8, device=dx.device)
        lib.check(L.plk_field_batch_inverse_dev(fid, dev._dp(dx), dev._dp(out), dev._dp(none), n, dev._stream()))
        assert torch.equal(dx, keep), n  # the input is only read
        assert words_to_ints(dev.to_host(out)) == want and np.array_equal(none.cpu().numpy(), flags), n
        out2 = torch.full_like(dx, 0x5A5A)
        lib.check(L.plk_field_batch_inverse_dev(fid, dev._dp(dx), dev._dp(out2), None, n, dev._stream()))
        assert torch.equal(out2, out), n
        none3 = torch.full((n,), 7, dtype=torch.uint8, device=dx.device)
        lib.check(L.plk_field_batch_inverse_dev(fid, dev._dp(dx), dev._dp(dx), dev._dp(none3), n, dev._stream()))
        assert torch.equal(dx, out) and torch.equal(none3, none), n


# =============================================================================================
# ProjectivePoint::batch_to_affine
# =============================================================================================
@functools.lru_cache(maxsize=None)
def multiples(cid):
    """k G for k = 1 .. max(N_BATCH), by repeated addition"""
    c = br.CURVES[cid]
    G = (c.gx, c.gy)
    pts = [G]
    for _ in range(max(N_BATCH) - 1):
        pts.append(br.ec_add(c, pts[-1], G))
    assert all(P is not None for P in pts) and br.ec_on_curve(c, pts[-1])
    return pts


IDENTITY_KINDS = ("flagged_garbage", "z0_unflagged", "flagged_z0")


@functools.lru_cache(maxsize=None)
def affine_inputs(cid, n):
    """-> ((n, 3, L) stored words, flags, expected (x, y, zero) with the flags, expected with proj_zero == NULL).  Real points are
    representatives (x z, y z, z) of k G with z among 1, p - 1 and random; the three kinds of identity are scattered among them, and from
    n = 4 on lane 0 holds a real point in every slot (the longest chain there is) next to lane 1 with an identity in every slot."""
    c = br.CURVES[cid]
    f, p = c.base, c.base.p
    rng = random.Random(0xAFF1 + 1000 * cid + n)
    pts = list(multiples(cid)[:n])
    kinds = ["real"] * n
    for i in range(n):
        if i % 11 == 5:
            kinds[i] = IDENTITY_KINDS[0]
        elif i % 13 == 7:
            kinds[i] = IDENTITY_KINDS[1]
        elif i % 17 == 3:
            kinds[i] = IDENTITY_KINDS[2]
    if n >= 4:
        for j, i in enumerate(chain(n, 1)):
            kinds[i] = IDENTITY_KINDS[j % 3]
        for i in chain(n, 0):
            kinds[i] = "real"
    if c is br.BLS12_377 and n > 2:
        pts[2], kinds[2] = (p - 1, 0), "real"  # the 2-torsion point: y = 0
    rows, flags, want, want_null = [], [], [], []
    for i in range(n):
        z = (1, p - 1, rng.randrange(2, p - 1))[rng.randrange(3)]
        if kinds[i] == "real":
            X, Y, Z, flag = pts[i][0] * z % p, pts[i][1] * z % p, z, 0
        else:
            X, Y = rng.randrange(1, p), rng.randrange(1, p)
            Z = z if kinds[i] == "flagged_garbage" else 0
            flag = 0 if kinds[i] == "z0_unflagged" else 1
        rows.append((X, Y, Z))
        flags.append(flag)
        zi = pow(Z, -1, p) if Z else 0
        value = (X * zi % p, Y * zi % p, 0)
        if kinds[i] == "real":
            assert value == (pts[i][0], pts[i][1], 0)
        want.append((0, 0, 1) if flag or not Z else value)
        want_null.append((0, 0, 1) if not Z else value)
    arr = ints_to_words([f.to_mont(v) for row in rows for v in row], f.n_limbs).reshape(n, 3, f.n_limbs)
    return arr, np.array(flags, dtype=np.uint8), want, want_null


def _check_affine(f, out, oz, want, where):
    assert [int(z) for z in oz] == [w[2] for w in want], where
    assert words_to_ints(out) == [f.to_mont(v) for w in want for v in w[:2]], where


@pytest.mark.parametrize("c", CURVES, ids=name)
def test_batch_to_affine_chains_and_identities(c):
    """Chains of 2 to 8 real points (n > 128), an unflagged Z = 0 (the identity), flagged entries with non-zero garbage and with Z = 0
    ((0, 0, zero)), a chain of identities beside a chain of real points, (-1, 0) on BLS12-377; with the flags and with proj_zero == NULL."""
    for n in N_BATCH:
        arr, flags, want, want_null = affine_inputs(c.curve_id, n)
        if n > 128:
            assert all(want[i][2] == 0 for i in chain(n, 0)) and all(want[i][2] == 1 for i in chain(n, 1)) and len(chain(n, 0)) >= 2
        out, oz = api.batch_to_affine(c.curve_id, arr, flags)
        _check_affine(c.base, out, oz, want, (n, "flags"))
        out, oz = api.batch_to_affine(c.curve_id, arr, None)
        _check_affine(c.base, out, oz, want_null, (n, "no flags"))


@pytest.mark.parametrize("c", CURVES, ids=name)
def test_batch_to_affine_dev_gives_the_host_entrys_words(c):
    torch, dev, lib = _gpu()
    L = lib.load()
    for n in N_DEV:
        arr, flags, want, want_null = affine_inputs(c.curve_id, n)
        dp, dz = dev.to_device(arr), torch.from_numpy(flags).to("cuda")
        for zero, expect in ((dz, want), (None, want_null)):
            host_xy, host_z = api.batch_to_affine(c.curve_id, arr, None if zero is None else flags)
            oxy = torch.full((n, 2, c.base.n_limbs), 0x5A5A, dtype=torch.int64, device="cuda")
            oz = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
            lib.check(L.plk_curve_batch_to_affine_dev(c.curve_id, n, dev._dp(dp), dev._dp(zero), dev._dp(oxy), dev._dp(oz), dev._stream()))
            assert np.array_equal(dev.to_host(oxy), host_xy) and np.array_equal(oz.cpu().numpy(), host_z), n
            _check_affine(c.base, dev.to_host(oxy), oz.cpu().numpy(), expect, n)


# =============================================================================================
# Field::inner_product and the folds of halo_a / halo_b
# =============================================================================================
def _inner_product(f, a, b):
    """-> (the device's word, the reference's) for host arrays a, b; the inputs must come back unchanged"""
    torch, dev, _ = _gpu()
    da, db = dev.to_device(a), dev.to_device(b)
    ka, kb = da.clone(), db.clone()
    out = dev.inner_product_dev(f.field_id, da, db)
    got = words_to_ints(dev.to_host(out))
    assert out.shape == (1, f.n_limbs) and torch.equal(da, ka) and torch.equal(db, kb)
    return got, [sum(x * y for x, y in zip(words_to_ints(a), words_to_ints(b))) * f.Rinv % f.p]


@pytest.mark.parametrize("f", FIELDS, ids=name)
def test_inner_product_at_block_edges_and_of_extreme_words(f):
    fid, L = f.field_id, f.n_limbs
    for n in IP_N:
        got, want = _inner_product(f, synth.rand_field(fid, 0x1A000000 + n, n), synth.rand_field(fid, 0x1B000000 + n, n))
        assert got == want and (n or got == [0]), n
    # all p - 1: as stored words (the largest operands the multiplier sees) and as the element -1
    for word, n in itertools.product((f.p - 1, f.to_mont(f.p - 1)), (257, 65537)):
        v = np.tile(ints_to_words([word], L), (n, 1))
        got, want = _inner_product(f, v, v)
        assert got == want and want == [n * word * word * f.Rinv % f.p], (word, n)


@pytest.mark.parametrize("f", [br.TWEEDLEDEE_BASE, br.BLS12_377_BASE], ids=name)
def test_inner_product_second_grid_stride_trip(f):
    n = IP_SECOND_TRIP
    got, want = _inner_product(f, synth.rand_field(f.field_id, 0x1C000000, n), synth.rand_field(f.field_id, 0x1D000000, n))
    assert got == want


@pytest.mark.parametrize("f", FIELDS, ids=name)
def test_fold_slices_out_of_place_and_onto_lo(f):
    """scalar_lo * lo + scalar_hi * hi for scalar pairs drawn from 0, 1, p - 1 and random, through device.fold_slices_dev and through the
    raw entry with d_out == d_lo (which the header allows)."""
    torch, dev, lib = _gpu()
    L = lib.load()
    fid, p = f.field_id, f.p
    rng = random.Random(0xF01D + fid)
    scalars = [0, 1, p - 1, rng.randrange(2, p - 1)]
    for n in FOLD_N:
        lo, hi = synth.rand_field(fid, 0x2A000000 + n, n), synth.rand_field(fid, 0x2B000000 + n, n)
        lo_i, hi_i = words_to_ints(lo), words_to_ints(hi)
        dlo, dhi = dev.to_device(lo), dev.to_device(hi)
        klo, khi = dlo.clone(), dhi.clone()
        for s_lo, s_hi in itertools.product(scalars, scalars):
            wl, wh = f.to_mont(s_lo), f.to_mont(s_hi)
            want = [(wl * x + wh * y) * f.Rinv % p for x, y in zip(lo_i, hi_i)]
            sl, sh = ints_to_words([wl], f.n_limbs)[0], ints_to_words([wh], f.n_limbs)[0]
            assert words_to_ints(dev.to_host(dev.fold_slices_dev(fid, dlo, dhi, sl, sh))) == want, (n, s_lo, s_hi)
            onto = dlo.clone()
            lib.check(L.plk_field_fold_slices_dev(fid, dev._dp(onto), dev._dp(dhi), dev._hp(sl), dev._hp(sh), n, dev._dp(onto), dev._stream()))
            assert words_to_ints(dev.to_host(onto)) == want, (n, s_lo, s_hi, "d_out == d_lo")
        assert torch.equal(dlo, klo) and torch.equal(dhi, khi), n


# =============================================================================================
# the byte encodings
# =============================================================================================
def _le_bytes(vals, size):
    return np.frombuffer(b"".join(int(v).to_bytes(size, "little") for v in vals), dtype=np.uint8).reshape(len(vals), size).copy()


@pytest.mark.parametrize("f", FIELDS, ids=name)
def test_field_bytes_round_trip_at_block_edges(f):
    fid, L, p = f.field_id, f.n_limbs, f.p
    for n in (127, 128, 129):
        x = synth.rand_field(fid, 0x5E710000 + n, n)
        x[[0, 1, n - 2, n - 1]] = ints_to_words([0, p - 1, f.to_mont(1), f.to_mont(p - 1)], L)  # canonical 0, (p - 1) / R, 1, p - 1
        want = _le_bytes([v * f.Rinv % p for v in words_to_ints(x)], 8 * L)
        b = api.field_to_bytes(fid, x)
        assert np.array_equal(b, want), n
        assert np.array_equal(api.field_from_bytes(fid, b), x), n


def range_records(f):
    """-> (values below p, values not below p): what canonical_in_range must tell apart, word by 32-bit word from the top"""
    p, bits = f.p, 64 * f.n_limbs
    top = bits - 32
    assert p & 0xFFFFFFFF == 1 and (p >> top) + 1 < 1 << 32
    good = [0, p - 1,
            p - 1,  # p with only the lowest word lowered by one (that word of p is 1): the comparison runs to its last word
            (((p >> top) - 1) << top) | ((1 << top) - 1)]  # the top word lowered, every other word 0xFFFFFFFF: settled by the first word
    bad = [p, p + 1, (1 << bits) - 1, p + (1 << top)]  # ..., p with only the top word raised by one
    assert all(v < p for v in good) and all(p <= v < 1 << bits for v in bad)
    return good, bad


@pytest.mark.parametrize("f", FIELDS, ids=name)
def test_field_from_bytes_range_check_counts_and_still_decodes(f):
    _, _, lib = _gpu()
    fid, L, p, n = f.field_id, f.n_limbs, f.p, 129
    good, bad = range_records(f)
    vals = [v * f.Rinv % p for v in words_to_ints(synth.rand_field(fid, 0x5E720000, n))]
    spots = [0, 1, 63, 64, 65, 126, 127, 128]
    for i, v in zip(spots, [v for pair in zip(bad, good) for v in pair]):
        vals[i] = v
    b = _le_bytes(vals, 8 * L)
    out = np.full((n, L), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    rc = lib.load().plk_field_from_bytes(fid, api._ptr(b), n, api._ptr(out))
    text = lib.load().plk_last_error().decode()
    assert rc == lib.PLK_ERR_INVALID_ARG and text.startswith("Out of range: %d of the %d records" % (len(bad), n)), text
    assert words_to_ints(out) == [f.to_mont(v) if v < p else 0 for v in vals]  # the good records of the same call still decode
    assert ol.field_from_bytes(fid, b)[1] == len(bad)
    with pytest.raises(ValueError, match="Out of range: %d of the %d records" % (len(bad), n)):
        api.field_from_bytes(fid, b)
    ok = [i for i in range(n) if vals[i] < p]
    assert words_to_ints(api.field_from_bytes(fid, b[ok])) == [f.to_mont(vals[i]) for i in ok]


def point_records(c, n):
    """-> [(mask, x as the integer its bytes hold)]: k G under masks 0 .. 3 (bit 1: which root; bit 0: the identity, whatever x says) and, at
    both ends of the call, an identity whose x bytes are not below p, x = 0, x not below p, an x with no point above it and, on
    BLS12-377, the 2-torsion point x = p - 1 (x^3 + B = 0: r = 0 and -r = 0) under both parities"""
    f, p = c.base, c.base.p
    full = (1 << (64 * f.n_limbs)) - 1
    no_point = next(x for x in range(2, 100) if pow((x ** 3 + c.b) % p, (p - 1) // 2, p) == p - 1)
    recs = [(k % 4, multiples(c.curve_id)[k][0]) for k in range(n)]
    special = [(1, p), (3, full), (0, 0), (2, 0), (0, p), (2, p + 1), (0, no_point), (2, no_point)]
    if c is br.BLS12_377:
        special += [(0, p - 1), (2, p - 1)]
    for j, rec in enumerate(special):
        recs[n - 1 - j // 2 if j % 2 == 0 else j // 2] = rec
    return recs


def decode_by_integers(c, mask, xv):
    """serialization.rs:47-72 -> (x, y, zero, status)"""
    f, p = c.base, c.base.p
    if mask & 1:
        return 0, 0, 1, 0
    if xv >= p:
        return 0, 0, 0, 1
    root, _ = sc.restated_sqrt(f, (xv ** 3 + c.b) % p)
    if root is None:
        return 0, 0, 0, 2
    y = root if root & 1 == (mask & 2) >> 1 else (p - root) % p
    assert (y * y - xv ** 3 - c.b) % p == 0 and (y == 0 or y & 1 == (mask & 2) >> 1)
    return xv, y, 0, 0


@pytest.mark.parametrize("c", CURVES, ids=name)
def test_point_from_bytes_masks_edges_and_statuses(c):
    f, L, p = c.base, c.base.n_limbs, c.base.p
    for n in (63, 64, 65):
        recs = point_records(c, n)
        want = [decode_by_integers(c, m, xv) for m, xv in recs]
        b = np.concatenate([np.array([[m] for m, _ in recs], dtype=np.uint8), _le_bytes([xv for _, xv in recs], 8 * L)], axis=1)
        xy, zero, status = api.point_from_bytes(c.curve_id, b, with_status=True)
        assert [int(s) for s in status] == [w[3] for w in want] and [int(z) for z in zero] == [w[2] for w in want], n
        assert words_to_ints(xy) == [f.to_mont(v) for w in want for v in w[:2]], n
        if c is br.BLS12_377:  # x = p - 1 under mask 0 and under mask 2: y = 0, status 0
            torsion = [w for (m, xv), w in zip(recs, want) if xv == p - 1]
            assert torsion == [(p - 1, 0, 0, 0)] * 2
        o_xy, o_zero, o_status = ol.point_from_bytes(c.curve_id, b, L)
        assert np.array_equal(o_status, status) and np.array_equal(o_zero, zero), n
        decoded = status == 0
        assert np.array_equal(o_xy[decoded], xy[decoded]) and decoded.sum() > n // 2, n
        # bits 2 .. 7 of the mask byte are not looked at
        high = b.copy()
        high[:, 0] |= 0xFC
        xy2, zero2, status2 = api.point_from_bytes(c.curve_id, high, with_status=True)
        assert np.array_equal(xy2, xy) and np.array_equal(zero2, zero) and np.array_equal(status2, status), n
        refused = int((status != 0).sum())
        with pytest.raises(ValueError, match="^%d of the %d points do not decode" % (refused, n)):
            api.point_from_bytes(c.curve_id, b)
        back, bz = api.point_from_bytes(c.curve_id, b[decoded])
        assert np.array_equal(back, xy[decoded]) and np.array_equal(bz, zero[decoded]), n


@pytest.mark.parametrize("c", CURVES, ids=name)
def test_point_to_bytes_mask_of_a_flagged_point_keeps_the_parity_bit(c):
    """serialization.rs:34-40: mask = zero | odd, so a flagged point with an odd y is written with mask 3"""
    f, L = c.base, c.base.n_limbs
    for n in (63, 64, 65, 127, 128, 129):
        pts = multiples(c.curve_id)[:n]
        flags = np.array([1 if k % 3 == 0 else 0 for k in range(n)], dtype=np.uint8)
        xy = ints_to_words([f.to_mont(v) for P in pts for v in P], L).reshape(n, 2, L)
        want_mask = [int(z) | (P[1] & 1) << 1 for z, P in zip(flags, pts)]
        assert {0, 1, 2, 3} <= set(want_mask)
        b = api.point_to_bytes(c.curve_id, xy, flags)
        assert [int(m) for m in b[:, 0]] == want_mask, n
        assert np.array_equal(b[:, 1:], _le_bytes([P[0] for P in pts], 8 * L)), n
        assert np.array_equal(b, ol.point_to_bytes(c.curve_id, xy, flags)), n
