"""GPU tests of the opening step (opening.hip): plk_field_powers, plk_plonk_eval_polys, plk_poly_reduce, plk_halo_build_b, plk_halo_s
and their _dev forms.  Everything is exact field arithmetic, so every comparison is bit for bit.

References are written here on Python integers: Horner for the opened values, pow for powers and halo_b, the literal double loop for
the reduction (halo.rs:39-44), the literal loop of halo_s (plonk_util.rs:311-326).  Stored words are Montgomery form (value * 2^256 mod p);
sums of stored words times canonical scalars are stored words again, so the references work on the stored words directly.

Kernel geometry the boundary sets are named after (opening.hip): the evaluation works on tiles of OPEN_TILE = 6144 coefficients, 256
lanes with 24 coefficients each in 4 rows of 6 (row boundaries every 1536 coefficients); the reduction and the generated vectors (powers,
halo_b, halo_s) run one element per lane in workgroups of 256, and the generated vectors split the index at 2^10 (two-level tables).
"""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from tests import checked_child

FIELDS = [br.TWEEDLEDEE_BASE, br.TWEEDLEDUM_BASE, br.BLS12_377_SCALAR, br.PALLAS_BASE, br.VESTA_BASE]
SMALL_N = [0, 1, 2, 3, 255, 256, 257, 1000, 1 << 12, (1 << 12) + 1]
OPEN_TILE, OPEN_ROW, LANES, LO = 6144, 1536, 256, 1024
RANDOM_INDICES = 4096
R = 1 << 256


# ---- stored words <-> Python integers ----
def words_to_ints(arr):
    b = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def ints_to_words(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(len(vals), 4).copy()


def mont(f, v):
    return v % f.p * R % f.p


def scalar_words(f, vals):
    return ints_to_words([mont(f, v) for v in vals])


# ---- the references, on stored words (ints) and canonical scalars ----
def ref_eval(f, c, x):
    """eval_from_power(powers(x, len)) = sum_j c[j] x^j, by Horner"""
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % f.p
    return acc


def ref_reduce(f, polys, scalars, degree):
    out = [0] * degree
    for s, c in zip(scalars, polys):  # halo.rs:39-44
        for j, v in enumerate(c):
            out[j] = (out[j] + s * v) % f.p
    return out


def ref_b_at(f, points, v, j):
    """reduce_with_powers([x^j for x in points], v), as a stored word"""
    acc = 0
    for x in reversed(points):
        acc = (acc * v + pow(x, j, f.p)) % f.p
    return mont(f, acc)


def ref_halo_s(f, us):
    p, k = f.p, len(us)
    res = [1] * (1 << k)
    inv = [pow(u, -1, p) for u in us]
    for j, (u, u_inv) in enumerate(zip(reversed(us), reversed(inv))):  # plonk_util.rs:316-324
        for i in range(len(res)):
            res[i] = res[i] * (u_inv if i & (1 << j) == 0 else u) % p
    return [mont(f, v) for v in res]


def ref_halo_s_at(f, us, i):
    p, k = f.p, len(us)
    acc = 1
    for j in range(k):
        u = us[k - 1 - j]
        acc = acc * (u if (i >> j) & 1 else pow(u, -1, p)) % p
    return mont(f, acc)


# ---- inputs ----
def edge_points(f, rng, count):
    """scalars including 0, 1, p - 1 and a root of unity"""
    pool = [0, 1, f.p - 1, f.primitive_root_of_unity(5), rng.randrange(f.p), 2, rng.randrange(f.p), f.primitive_root_of_unity(13)]
    start = rng.randrange(len(pool))
    return [pool[(i + start) % len(pool)] for i in range(count)]


def small_poly(f, rng, n):
    """n stored words: random values with planted edge words (the stored word 0 / 1 / p - 1 and the stored forms of those values)"""
    c = [rng.randrange(f.p) for _ in range(n)]
    edges = [0, 1, f.p - 1, mont(f, 1), mont(f, f.p - 1)]
    for t in range(min(n, 12)):
        c[rng.randrange(n)] = edges[t % len(edges)]
    if n:
        c[-1] = edges[(n + 1) % len(edges)]
        c[0] = edges[n % len(edges)]
    return c


def small_cases(f, seed):
    """(polys, points) of the small set: every n of SMALL_N as the leading length; 1, 3 and 8 points; 1, 2, 30 and 257 polynomials of mixed lengths"""
    rng = random.Random(seed)
    cases = []
    for idx, n in enumerate(SMALL_N):
        for n_points, n_polys in ((1, 1), (3, 2), (8, 30), (3, 30), (8, 2), (1, 30))[idx % 2::2] + ((3, 1),):
            lens = [n] + [SMALL_N[(idx + 3 * i + n_points) % len(SMALL_N)] for i in range(1, n_polys)]
            cases.append(([small_poly(f, rng, m) for m in lens], edge_points(f, rng, n_points)))
    for n_points in (3, 8):
        lens = [SMALL_N[(7 * i + n_points) % 8] for i in range(257)]  # 257 polynomials, lengths 0 .. 1000
        lens[100] = (1 << 12) + 1
        cases.append(([small_poly(f, rng, m) for m in lens], edge_points(f, rng, n_points)))
    # beyond the issue's lengths: the tile tail of the evaluation (OPEN_TILE - 1, OPEN_TILE, OPEN_TILE + 1, two tiles and one coefficient)
    cases.append(([small_poly(f, rng, m) for m in (OPEN_TILE - 1, OPEN_TILE, OPEN_TILE + 1, 2 * OPEN_TILE + 1, 0, 3)], edge_points(f, rng, 3)))
    cases.append(([small_poly(f, rng, m) for m in (2 * OPEN_TILE + 1, OPEN_TILE + 1)], edge_points(f, rng, 8)))
    return cases


def dev_polys(dev, polys):
    return [dev.to_device(ints_to_words(c) if c else np.zeros((0, 4), dtype=np.uint64)) for c in polys]


def run_small_set(fields=FIELDS, host_twins=True):
    """The small, exhaustive set on the loaded library: every output of every entry against the references; host twins against the
    _dev entries; inputs unchanged.  Returns the number of compared outputs."""
    import torch
    from plonky_amd import api, device as dev
    dev.init(0)
    compared = 0
    for f in fields:
        fid, p = f.field_id, f.p
        rng = random.Random(0x0DE7 + fid)
        for polys, points in small_cases(f, 0x5EED + fid):
            d = dev_polys(dev, polys)
            before = [t.clone() for t in d]
            pw = scalar_words(f, points)
            got = dev.to_host(dev.eval_polys_dev(fid, d, pw))
            exp = [[ref_eval(f, c, x) for c in polys] for x in points]
            assert words_to_ints(got) == [v for row in exp for v in row], (f.name, len(polys), len(points))
            compared += len(polys) * len(points)
            degree = max(len(c) for c in polys) + (len(polys) % 3)
            scalars = [edge_points(f, rng, 8)[i % 8] if i % 5 else rng.randrange(p) for i in range(len(polys))]
            sw = scalar_words(f, scalars)
            red = dev.to_host(dev.reduce_polynomials_dev(fid, d, sw, degree))
            assert words_to_ints(red) == ref_reduce(f, polys, scalars, degree), (f.name, len(polys), degree)
            compared += degree
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(before, d)), "inputs changed"
            if host_twins:
                arrs = [ints_to_words(c) if c else np.zeros((0, 4), dtype=np.uint64) for c in polys]
                assert np.array_equal(api.eval_polys(fid, arrs, pw), got)
                assert np.array_equal(api.reduce_polynomials(fid, arrs, sw, degree), red)
        for n in SMALL_N:
            for x in (0, 1, p - 1, f.primitive_root_of_unity(5), rng.randrange(p)):
                xw = scalar_words(f, [x])[0]
                got = dev.to_host(dev.powers_dev(fid, xw, n))
                assert words_to_ints(got) == [mont(f, pow(x, j, p)) for j in range(n)], (f.name, n, x)
                compared += n
                if host_twins:
                    assert np.array_equal(api.powers(fid, xw, n), got)
            for n_points in (1, 3, 8):
                pts, v = edge_points(f, rng, n_points), (0, 1, p - 1, rng.randrange(p))[(n + n_points) % 4]
                got = dev.to_host(dev.build_halo_b_dev(fid, scalar_words(f, pts), scalar_words(f, [v])[0], n))
                assert words_to_ints(got) == [ref_b_at(f, pts, v, j) for j in range(n)], (f.name, n, n_points)
                compared += n
                if host_twins:
                    assert np.array_equal(api.build_halo_b(fid, scalar_words(f, pts), scalar_words(f, [v])[0], n), got)
        for k in range(0, 11):
            us = [(1, p - 1, f.primitive_root_of_unity(7))[i] if i < 3 and k % 2 else rng.randrange(1, p) for i in range(k)]
            uw = scalar_words(f, us) if k else np.zeros((0, 4), dtype=np.uint64)
            got = dev.to_host(dev.halo_s_dev(fid, uw))
            assert words_to_ints(got) == ref_halo_s(f, us), (f.name, k)
            compared += 1 << k
            if host_twins:
                assert np.array_equal(api.halo_s(fid, uw), got)
    return compared


@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_small_exhaustive(f):
    assert run_small_set([f]) > 0


# ---- full size ----
def device_words(f, shape, gen):
    """int64 CUDA tensor shape + (4,): independent canonical stored words (top limb masked below the top bit of p)"""
    import torch
    t = torch.randint(-(1 << 31), 1 << 31, tuple(shape) + (8,), dtype=torch.int32, device="cuda", generator=gen).view(torch.int64)
    t[..., 3] &= (1 << (f.p.bit_length() - 1 - 192)) - 1
    return t


def full_polys(f, log_n, seed, count=30):
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return [device_words(f, (1 << log_n,), gen) for _ in range(count)]


def oracle_inner_product(fid, a, b):
    """Field::inner_product (field.rs:213-221) through the oracle's field arithmetic: its products, added up pairwise (the order does not matter)"""
    from oracle import oracle_lib as ol
    acc = ol.field_binop(fid, "mul", a, b)
    while acc.shape[0] > 1:
        if acc.shape[0] % 2:
            acc = np.concatenate([acc, np.zeros((1, 4), dtype=np.uint64)])
        h = acc.shape[0] // 2
        acc = ol.field_binop(fid, "add", np.ascontiguousarray(acc[:h]), np.ascontiguousarray(acc[h:]))
    return acc[0]


def python_powers(f, x, n):
    """powers(x, n) as stored words, made by Python integers"""
    out, cur = [], mont(f, 1)
    for _ in range(n):
        out.append(cur)
        cur = cur * x % f.p
    return ints_to_words(out)


FULL = [(f, 20) for f in FIELDS] + [(br.TWEEDLEDUM_BASE, 22)]


@pytest.mark.parametrize("f,log_n", FULL, ids=lambda v: v.name if hasattr(v, "name") else "n%d" % v)
def test_full_size_values_against_oracle_inner_product(f, log_n):
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    fid, n = f.field_id, 1 << log_n
    polys = full_polys(f, log_n, 0xA11 + fid + log_n)
    before = [int(t.sum()) for t in polys]
    rng = random.Random(0xFACE + fid)
    points = [rng.randrange(f.p) for _ in range(3)]
    got = dev.to_host(dev.eval_polys_dev(fid, polys, scalar_words(f, points)))
    pws = [python_powers(f, x, n) for x in points]
    for i, t in enumerate(polys):
        c = dev.to_host(t)
        for k in range(3):
            assert np.array_equal(got[k, i], oracle_inner_product(fid, c, pws[k])), (f.name, i, k)
    torch.cuda.synchronize()
    assert before == [int(t.sum()) for t in polys], "inputs changed"


@pytest.mark.parametrize("f,log_n", FULL, ids=lambda v: v.name if hasattr(v, "name") else "n%d" % v)
def test_full_size_values_against_ntt(f, log_n):
    """At the points w^j of the size-n subgroup the value of polynomial i is entry j of its transform.  The points are read from the transform
    of the polynomial X, so neither the root nor the output order is assumed."""
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    fid, n = f.field_id, 1 << log_n
    polys = full_polys(f, log_n, 0xB22 + fid + log_n)
    x_poly = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    x_poly[1] = dev.to_device(scalar_words(f, [1]))[0]
    x_values = dev.ntt_dev(fid, x_poly)
    js = [1, n // 2 + 3, n - 1]
    points = dev.to_host(x_values[js])
    assert len({tuple(r) for r in points.tolist()}) == 3
    got = dev.eval_polys_dev(fid, polys, points)
    for i, t in enumerate(polys):
        values = dev.ntt_dev(fid, t)
        assert torch.equal(values[js], got[:, i]), (f.name, i)


def boundary_indices(n, extra=()):
    """first, last, and both sides of every workgroup (256), row (1536), tile (6144) and table (1024) boundary below n"""
    s = {0, 1, n - 2, n - 1}
    for step in (LANES, LO, OPEN_ROW, OPEN_TILE):
        for b in range(step, n, step):
            s |= {b - 1, b}
    for e in extra:
        s |= {e - 1, e, e + 1}
    return sorted(i for i in s if 0 <= i < n)


def sampled(n, seed, extra=()):
    rng = random.Random(seed)
    idx = boundary_indices(n, extra) + [rng.randrange(n) for _ in range(RANDOM_INDICES)]
    return idx


@pytest.mark.parametrize("f,log_n", FULL, ids=lambda v: v.name if hasattr(v, "name") else "n%d" % v)
def test_full_size_reduction_b_powers_and_identity(f, log_n):
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    fid, n, p = f.field_id, 1 << log_n, f.p
    polys = full_polys(f, log_n, 0xC33 + fid + log_n)
    lens = [n] * 30
    lens[3], lens[7], lens[11] = n - 1, n // 2 + 77, 5000  # zero-padded ones among them
    polys = [t[:m].contiguous() for t, m in zip(polys, lens)]
    rng = random.Random(0xD44 + fid)
    scalars = [rng.randrange(p) for _ in range(30)]
    scalars[5], scalars[6] = 0, p - 1
    points = [rng.randrange(p) for _ in range(3)]
    v = rng.randrange(p)
    halo_a = dev.reduce_polynomials_dev(fid, polys, scalar_words(f, scalars), n)
    halo_b = dev.build_halo_b_dev(fid, scalar_words(f, points), scalar_words(f, [v])[0], n)
    pw = dev.powers_dev(fid, scalar_words(f, [points[0]])[0], n)
    idx = sampled(n, 0xE55 + fid, extra=lens)
    assert len(idx) >= RANDOM_INDICES + 2 * (n // LANES - 1)
    it = torch.tensor(idx, device="cuda")
    cols = []
    for t in polys:
        col = torch.zeros((len(idx), 4), dtype=torch.int64, device="cuda")
        inside = it < t.shape[0]
        col[inside] = t[it[inside]]
        cols.append(words_to_ints(dev.to_host(col)))
    exp_a = [sum(s * c[r] for s, c in zip(scalars, cols)) % p for r in range(len(idx))]
    assert words_to_ints(dev.to_host(halo_a[it])) == exp_a
    assert words_to_ints(dev.to_host(halo_b[it])) == [ref_b_at(f, points, v, j) for j in idx]
    assert words_to_ints(dev.to_host(pw[it])) == [mont(f, pow(points[0], j, p)) for j in idx]
    # <halo_a, halo_b> = sum_k v^k sum_i s_i o[k][i]   (halo.rs:38-47: the opened values of the reduced polynomial)
    if log_n == 20:
        full = [t if t.shape[0] == n else torch.cat([t, torch.zeros((n - t.shape[0], 4), dtype=torch.int64, device="cuda")]) for t in polys]
        o = words_to_ints(dev.to_host(dev.eval_polys_dev(fid, polys, scalar_words(f, points))))
        o_padded = words_to_ints(dev.to_host(dev.eval_polys_dev(fid, full, scalar_words(f, points))))
        assert o == o_padded
        rhs = sum(pow(v, k, p) * sum(s * o[k * 30 + i] for i, s in enumerate(scalars)) for k in range(3)) % p
        lhs = words_to_ints(dev.to_host(dev.inner_product_dev(fid, halo_a, halo_b)))[0]
        assert lhs == rhs


@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_halo_s_at_k20(f):
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    rng = random.Random(0xF66 + f.field_id)
    us = [rng.randrange(1, f.p) for _ in range(20)]
    got = dev.halo_s_dev(f.field_id, scalar_words(f, us))
    idx = sampled(1 << 20, 0x177 + f.field_id)
    assert words_to_ints(dev.to_host(got[torch.tensor(idx, device="cuda")])) == [ref_halo_s_at(f, us, i) for i in idx]


# ---- calling conventions ----
def test_same_polynomial_twice_out_argument_and_side_stream():
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    f = br.TWEEDLEDUM_BASE
    fid, n = f.field_id, 1 << 16
    rng = random.Random(0x288)
    points, scalars, v = [rng.randrange(f.p) for _ in range(3)], [rng.randrange(f.p) for _ in range(3)], rng.randrange(f.p)
    pw, sw = scalar_words(f, points), scalar_words(f, scalars)
    a, b = full_polys(f, 16, 0x299, count=2)
    # the same polynomial passed twice
    vals = dev.eval_polys_dev(fid, [a, b, a], pw)
    assert torch.equal(vals[:, 0], vals[:, 2])
    red = dev.reduce_polynomials_dev(fid, [a, b, a], sw, n)
    both = scalar_words(f, [scalars[0] + scalars[2], scalars[1]])
    assert torch.equal(red, dev.reduce_polynomials_dev(fid, [a, b], both, n))
    # outputs into a caller's out=
    outs = {"vals": torch.zeros_like(vals), "red": torch.zeros_like(red), "b": torch.zeros((n, 4), dtype=torch.int64, device="cuda"),
            "pw": torch.zeros((n, 4), dtype=torch.int64, device="cuda"), "s": torch.zeros((1 << 12, 4), dtype=torch.int64, device="cuda")}
    us = scalar_words(f, [rng.randrange(1, f.p) for _ in range(12)])
    assert dev.eval_polys_dev(fid, [a, b, a], pw, out=outs["vals"]) is outs["vals"] and torch.equal(outs["vals"], vals)
    assert dev.reduce_polynomials_dev(fid, [a, b, a], sw, n, out=outs["red"]) is outs["red"] and torch.equal(outs["red"], red)
    assert torch.equal(dev.build_halo_b_dev(fid, pw, sw[0], n, out=outs["b"]), dev.build_halo_b_dev(fid, pw, sw[0], n))
    assert torch.equal(dev.powers_dev(fid, pw[0], n, out=outs["pw"]), dev.powers_dev(fid, pw[0], n))
    assert torch.equal(dev.halo_s_dev(fid, us, out=outs["s"]), dev.halo_s_dev(fid, us))
    # a side stream: the calls are enqueued behind the kernel that produces their input, with no synchronisation between
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        values = dev.ntt_dev(fid, a, inverse=True)          # the producer
        s_vals = dev.eval_polys_dev(fid, [values, b], pw)
        s_red = dev.reduce_polynomials_dev(fid, [values, b], sw[:2], n)
        s_b = dev.build_halo_b_dev(fid, pw, sw[0], n)
        s_ip = dev.inner_product_dev(fid, s_red, s_b)
    side.synchronize()
    values2 = dev.ntt_dev(fid, a, inverse=True)
    torch.cuda.synchronize()
    assert torch.equal(values, values2)
    assert torch.equal(s_vals, dev.eval_polys_dev(fid, [values2, b], pw))
    assert torch.equal(s_red, dev.reduce_polynomials_dev(fid, [values2, b], sw[:2], n))
    assert torch.equal(s_b, outs["b"])
    assert torch.equal(s_ip, dev.inner_product_dev(fid, s_red, s_b))


def test_argument_errors():
    """null pointer, lens[i] > degree, zero in us, n_points 0 or 9: an error code, a plk_last_error text, outputs untouched"""
    import torch
    from plonky_amd import api, device as dev, lib
    dev.init(0)
    L = lib.load()
    f = br.TWEEDLEDUM_BASE
    fid = f.field_id
    a = dev.to_device(ints_to_words(list(range(1, 101))))
    ptrs = (ctypes.c_void_p * 2)(a.data_ptr(), a.data_ptr())
    nulls = (ctypes.c_void_p * 2)(a.data_ptr(), None)
    lens = np.array([100, 100], dtype=np.uint64)
    sc = scalar_words(f, [3, 4, 5, 6, 7, 8, 9, 10, 11])
    out = torch.full((1024, 4), 0x5A5A, dtype=torch.int64, device="cuda")
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    o = ctypes.c_void_p(out.data_ptr())

    def refused(rc, word=None):
        assert rc == lib.PLK_ERR_INVALID_ARG, rc
        text = L.plk_last_error().decode()
        assert text and (word is None or word in text), text

    for n_points in (0, 9):
        refused(L.plk_plonk_eval_polys_dev(fid, 2, ptrs, vp(lens), n_points, vp(sc), o, None), "n_points")
        refused(L.plk_halo_build_b_dev(fid, n_points, vp(sc), vp(sc), 100, o, None), "n_points")
        refused(L.plk_plonk_eval_polys(fid, 0, None, None, n_points, vp(sc), None), "n_points")
        refused(L.plk_halo_build_b(fid, n_points, vp(sc), vp(sc), 0, None), "n_points")
    refused(L.plk_plonk_eval_polys_dev(fid, 2, nulls, vp(lens), 3, vp(sc), o, None), "null")
    refused(L.plk_plonk_eval_polys_dev(fid, 2, ptrs, vp(lens), 3, None, o, None), "null")
    refused(L.plk_plonk_eval_polys_dev(fid, 2, ptrs, vp(lens), 3, vp(sc), None, None), "null")
    refused(L.plk_plonk_eval_polys_dev(fid, 2, None, vp(lens), 3, vp(sc), o, None), "null")
    refused(L.plk_poly_reduce_dev(fid, 2, nulls, vp(lens), vp(sc), 100, o, None), "null")
    refused(L.plk_poly_reduce_dev(fid, 2, ptrs, vp(lens), None, 100, o, None), "null")
    refused(L.plk_poly_reduce_dev(fid, 2, ptrs, vp(lens), vp(sc), 100, None, None), "null")
    refused(L.plk_poly_reduce_dev(fid, 2, ptrs, vp(lens), vp(sc), 99, o, None), "more than the degree")
    refused(L.plk_halo_build_b_dev(fid, 3, None, vp(sc), 100, o, None), "null")
    refused(L.plk_halo_build_b_dev(fid, 3, vp(sc), None, 100, o, None), "null")
    refused(L.plk_halo_build_b_dev(fid, 3, vp(sc), vp(sc), 100, None, None), "null")
    refused(L.plk_field_powers_dev(fid, None, 100, o, None), "null")
    refused(L.plk_field_powers_dev(fid, vp(sc), 100, None, None), "null")
    refused(L.plk_halo_s_dev(fid, 3, None, o, None), "null")
    refused(L.plk_halo_s_dev(fid, 3, vp(sc), None, None), "null")
    refused(L.plk_halo_s_dev(fid, 31, vp(sc), o, None))
    refused(L.plk_plonk_eval_polys_dev(3, 2, ptrs, vp(lens), 3, vp(sc), o, None), "field")  # Bls12377Base: six limbs
    with_zero = scalar_words(f, [3, 0, 5])
    rc = L.plk_halo_s_dev(fid, 3, vp(with_zero), o, None)
    assert rc == lib.PLK_ERR_INVALID_ARG and L.plk_last_error().decode().startswith("No inverse")
    host_out = np.zeros((8, 4), dtype=np.uint64)
    rc = L.plk_halo_s(fid, 3, vp(with_zero), vp(host_out))
    assert rc == lib.PLK_ERR_INVALID_ARG and L.plk_last_error().decode().startswith("No inverse")
    with pytest.raises(AssertionError, match="No inverse"):
        api.halo_s(fid, with_zero)
    with pytest.raises(AssertionError):
        api.reduce_polynomials(fid, [dev.to_host(a)], sc[:1], 99)
    harr = dev.to_host(a)
    hp = (ctypes.c_void_p * 1)(harr.ctypes.data)
    refused(L.plk_poly_reduce(fid, 1, hp, vp(lens), vp(sc), 99, vp(np.zeros((99, 4), dtype=np.uint64))), "more than the degree")
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A).all()), "a refused call wrote to its output"
    # and the library still works
    assert words_to_ints(dev.to_host(dev.powers_dev(fid, sc[0], 3))) == [mont(f, 1), mont(f, 3), mont(f, 9)]


CHECKED_BODY = '''
from tests.test_gpu_opening import run_small_set
print("CHECKED compared", run_small_set())
'''


def test_checked_build_runs_the_small_set():
    assert "CHECKED compared" in checked_child.run_checked(CHECKED_BODY, timeout=1200)
