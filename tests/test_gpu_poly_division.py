"""GPU tests of the low-degree polynomial division (polydiv.hip): plk_poly_division_dev, plk_poly_division, plk_poly_from_roots, the
mirrors in api.py (polynomial_division, polynomial_long_division, polynomial_from_roots, scale_polynomials) and
device.public_input_quotient_dev.  The field is exact and quotient and remainder are unique: every comparison is bit for bit.

The reference is long division on Python integers, written here: stored words (value * 2^256 mod p) -> canonical values, schoolbook
division, -> stored words.

Kernel geometry the boundary sets are named after (polydiv_step.cuh): a is cut into segments of S = 256 coefficients, a group of
k' = next power of two >= k lanes per segment; the scan takes blocks of B = 64 segments, so a with more than S * B coefficients is
the first to need the second scan level; divisors of degree above LAZY = 8 take the step that reduces every time.
"""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from tests import checked_child

FIELDS = [br.TWEEDLEDEE_BASE, br.TWEEDLEDUM_BASE, br.BLS12_377_SCALAR, br.PALLAS_BASE, br.VESTA_BASE]
S, B, LAZY, MAX_DEGREE = 256, 64, 8, 32
TWO_LEVEL = S * B + 1  # the first la with more than B segments
SHAPE = 2 * S + 7
DEGREES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32]
R = 1 << 256
F0 = br.TWEEDLEDUM_BASE  # Tweedledee's scalar field


# ---- stored words <-> Python integers ----
def words_to_ints(arr):
    b = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def ints_to_words(vals):
    if not len(vals):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(len(vals), 4).copy()


def stored(f, vals):
    return [v % f.p * R % f.p for v in vals]


def canonical(f, words):
    rinv = pow(R, -1, f.p)
    return [w * rinv % f.p for w in words]


# ---- the reference: schoolbook long division on canonical values (polynomial.rs:232-259) ----
def ref_divide(f, a, b):
    """a: la canonical values, b: k + 1 canonical values, b[k] != 0 -> (la - k quotient values, k remainder values)"""
    p, k = f.p, len(b) - 1
    inv = pow(b[k], -1, p)
    rem = list(a)
    q = [0] * (len(a) - k)
    for j in range(len(a) - k - 1, -1, -1):
        c = rem[j + k] * inv % p
        q[j] = c
        if c:
            for i in range(k + 1):
                rem[j + i] = (rem[j + i] - c * b[i]) % p
    return q, rem[:k]


def ref_divide_stored(f, a_words, b_words):
    q, r = ref_divide(f, canonical(f, a_words), canonical(f, b_words))
    return stored(f, q), stored(f, r)


def ref_mul(f, x, y):
    out = [0] * (len(x) + len(y) - 1)
    for i, u in enumerate(x):
        if u:
            for j, v in enumerate(y):
                out[i + j] = (out[i + j] + u * v) % f.p
    return out


def ref_from_roots(f, roots):
    c = [1]
    for r in roots:
        c = ref_mul(f, c, [(-r) % f.p, 1])
    return c


# ---- inputs ----
def rand_poly(f, rng, n):
    """n canonical values: random, with planted edge values (0, 1, p - 1 and the values whose stored words are 0 / 1 / p - 1)"""
    c = [rng.randrange(f.p) for _ in range(n)]
    rinv = pow(R, -1, f.p)
    edges = [0, 1, f.p - 1, rinv, (f.p - 1) * rinv % f.p]
    for t in range(min(n, 10)):
        c[rng.randrange(n)] = edges[t % len(edges)]
    return c


def rand_divisor(f, rng, k, lead=1):
    return rand_poly(f, rng, k) + [lead]


def divide_dev(f, a, b, q_len=None, with_rem=True):
    """a, b canonical values -> (q, rem) stored words as integers, through plk_poly_division_dev"""
    import torch
    from plonky_amd import device as dev, lib
    d_a = dev.to_device(ints_to_words(stored(f, a)))
    bw = ints_to_words(stored(f, b))
    k = len(b) - 1
    if q_len is None:
        q_len = len(a) - k
    q = torch.full((q_len, 4), -1, dtype=torch.int64, device="cuda")
    rem = torch.full((k, 4), -1, dtype=torch.int64, device="cuda")
    lib.check(lib.load().plk_poly_division_dev(f.field_id, ctypes.c_void_p(d_a.data_ptr()), len(a), bw.ctypes.data_as(ctypes.c_void_p), len(b),
                                               ctypes.c_void_p(q.data_ptr()), q_len, ctypes.c_void_p(rem.data_ptr()) if with_rem else None,
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert words_to_ints(dev.to_host(d_a)) == stored(f, a), "the input was changed"
    return words_to_ints(dev.to_host(q)), words_to_ints(dev.to_host(rem))


def check_division(f, a, b, q_len=None):
    q, r = ref_divide(f, a, b)
    got_q, got_r = divide_dev(f, a, b, q_len)
    pad = (q_len if q_len is not None else len(q)) - len(q)
    assert got_q == stored(f, q) + [0] * pad
    assert got_r == stored(f, r)


@pytest.fixture(scope="module", autouse=True)
def _init():
    from plonky_amd import device as dev
    dev.init()


# ---- every group width, full and partly filled ----
@pytest.mark.parametrize("k", DEGREES)
def test_every_degree(k):
    rng = random.Random(100 + k)
    check_division(F0, rand_poly(F0, rng, SHAPE), rand_divisor(F0, rng, k))


def _lengths(k):
    return sorted({k + 1, k + 2, S - 1, S, S + 1, S + k, 2 * S + 1, TWO_LEVEL, TWO_LEVEL + 1})


@pytest.mark.parametrize("k", [1, 3, 32])
def test_lengths_around_the_segment_and_the_second_scan_level(k):
    rng = random.Random(200 + k)
    for la in _lengths(k):
        lead = 1 if la % 2 else rng.randrange(2, F0.p)
        check_division(F0, rand_poly(F0, rng, la), rand_divisor(F0, rng, k, lead))


@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_all_fields(f):
    rng = random.Random(300 + f.field_id)
    check_division(f, rand_poly(f, rng, SHAPE), rand_divisor(f, rng, 3))
    check_division(f, rand_poly(f, rng, SHAPE), rand_divisor(f, rng, 3, f.p - 1))


# ---- edge divisors ----
def test_edge_divisors():
    from plonky_amd import api
    f, rng = F0, random.Random(400)
    a = rand_poly(f, rng, SHAPE)
    check_division(f, a, rand_divisor(f, rng, 5, rng.randrange(2, f.p)))      # not monic
    check_division(f, a, rand_divisor(f, rng, 5, f.p - 1))                    # lead = p - 1
    check_division(f, a, rand_divisor(f, rng, 17, f.p - 1))
    for k in (1, 4, 9):                                                       # b = X^k: q is a shift, r the low k coefficients
        q, r = divide_dev(f, a, [0] * k + [1])
        assert q == stored(f, a[k:]) and r == stored(f, a[:k])
    root = rng.randrange(f.p)
    check_division(f, a, ref_from_roots(f, [root, root, root, 5]))            # a repeated root
    g = f.primitive_root_of_unity(12)                                         # the prover's form: subgroup elements, through plk_poly_from_roots
    roots = [pow(g, e, f.p) for e in (0, 1, 7, 4095)]
    b_words = api.polynomial_from_roots(f.field_id, ints_to_words(stored(f, roots)))
    b = canonical(f, words_to_ints(b_words))
    assert b == ref_from_roots(f, roots)
    check_division(f, a, b)


# ---- edge dividends ----
def test_edge_dividends():
    f, rng = F0, random.Random(500)
    for k in (3, 12):
        b = rand_divisor(f, rng, k, 1 if k == 3 else 7)
        lead_zeros = rand_poly(f, rng, SHAPE - 40) + [0] * 40                # leading zeros, across a segment's top and inside it
        check_division(f, lead_zeros, b)
        check_division(f, rand_poly(f, rng, S - 3) + [0] * (S + 3 + 5), b)   # a whole zero top segment
        q, r = divide_dev(f, [0] * SHAPE, b)                                  # a all zero
        assert q == [0] * (SHAPE - k) and r == [0] * k
        q0 = rand_poly(f, rng, SHAPE - k)
        exact = ref_mul(f, q0, b)
        q, r = divide_dev(f, exact, b)                                        # a = q0 b: the remainder is all zero
        assert q == stored(f, q0) and r == [0] * k
        r0 = rand_poly(f, rng, k - 1) + [f.p - 1]                             # deg r0 = k - 1
        with_rem = [(v + (r0[i] if i < k else 0)) % f.p for i, v in enumerate(exact)]
        q, r = divide_dev(f, with_rem, b)
        assert q == stored(f, q0) and r == stored(f, r0)


# ---- outputs ----
def test_q_len_tail_null_remainder_and_host_form():
    import torch
    from plonky_amd import device as dev, lib
    f, rng = F0, random.Random(600)
    L = lib.load()
    for k, la, q_len in ((3, SHAPE, 2 * SHAPE), (3, SHAPE, 3 * S + 1), (3, SHAPE, SHAPE), (17, S + 17, 4 * S), (2, 5, 6)):
        a, b = rand_poly(f, rng, la), rand_divisor(f, rng, k, 1 if k == 3 else 9)
        q, r = ref_divide(f, a, b)
        # the tail is zero, words beyond q_len in a larger buffer are untouched
        d_a = dev.to_device(ints_to_words(stored(f, a)))
        buf = torch.full((q_len + 9, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        got_q, got_r = dev.polynomial_division_dev(f.field_id, d_a, ints_to_words(stored(f, b)), out=buf[:q_len])
        host = dev.to_host(buf)
        assert words_to_ints(host[:q_len]) == stored(f, q) + [0] * (q_len - len(q))
        assert (host[q_len:] == np.uint64(0x5A5A5A5A5A5A5A5A)).all()
        assert words_to_ints(dev.to_host(got_r)) == stored(f, r)
        # d_rem null
        got_q2, _ = divide_dev(f, a, b, q_len, with_rem=False)
        assert got_q2 == stored(f, q) + [0] * (q_len - len(q))
        # the host-pointer form equals the _dev form
        aw, bw = ints_to_words(stored(f, a)), ints_to_words(stored(f, b))
        hq, hr = np.empty((q_len, 4), dtype=np.uint64), np.empty((k, 4), dtype=np.uint64)
        lib.check(L.plk_poly_division(f.field_id, aw.ctypes.data_as(ctypes.c_void_p), la, bw.ctypes.data_as(ctypes.c_void_p), k + 1,
                                      hq.ctypes.data_as(ctypes.c_void_p), q_len, hr.ctypes.data_as(ctypes.c_void_p)))
        assert np.array_equal(hq, host[:q_len]) and np.array_equal(hr, dev.to_host(got_r))
        lib.check(L.plk_poly_division(f.field_id, aw.ctypes.data_as(ctypes.c_void_p), la, bw.ctypes.data_as(ctypes.c_void_p), k + 1,
                                      hq.ctypes.data_as(ctypes.c_void_p), q_len, None))
        assert np.array_equal(hq, host[:q_len])


@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_poly_from_roots(f):
    from plonky_amd import api
    rng = random.Random(700 + f.field_id)
    for k in (0, 1, 2, 32):
        roots = [rng.randrange(f.p) for _ in range(k)]
        if k == 32:
            roots[5] = roots[6] = roots[31]  # duplicate roots
            roots[0] = 0                     # a zero root
            roots[1] = f.p - 1
        got = api.polynomial_from_roots(f.field_id, ints_to_words(stored(f, roots)))
        assert got.shape == (k + 1, 4)
        assert words_to_ints(got) == stored(f, ref_from_roots(f, roots))
    assert words_to_ints(api.polynomial_from_roots(f.field_id, ints_to_words(stored(f, [0, 0])))) == stored(f, [0, 0, 1])


# ---- the mirrors ----
def test_mirrors_have_the_reference_lengths_in_every_branch():
    from plonky_amd import api
    f, rng = F0, random.Random(800)
    fid = f.field_id
    w = lambda vals: ints_to_words(stored(f, vals))
    for div in (api.polynomial_division, api.polynomial_long_division):
        # zero a -> ([0], empty)
        q, r = div(fid, w([0, 0, 0]), w([1, 2]))
        assert words_to_ints(q) == [0] and r.shape == (0, 4)
        # deg a < deg b -> ([0], a)
        a = [3, 4, 0]
        q, r = div(fid, w(a), w([1, 2, 3, 4]))
        assert words_to_ints(q) == [0] and words_to_ints(r) == stored(f, a)
        # otherwise: q and r trimmed, untrimmed inputs allowed
        a, b = rand_poly(f, rng, 700) + [0, 0], rand_divisor(f, rng, 6, 11) + [0]
        eq, er = ref_divide(f, a[:700], b[:7])
        while er and er[-1] == 0:
            er.pop()
        q, r = div(fid, w(a), w(b))
        assert words_to_ints(q) == stored(f, eq) and words_to_ints(r) == stored(f, er)
        # an exact division: the remainder is empty
        q0 = rand_poly(f, rng, 300)[:-1] + [5]
        q, r = div(fid, w(ref_mul(f, q0, b[:7])), w(b))
        assert words_to_ints(q) == stored(f, q0) and r.shape == (0, 4)
        # a zero b raises as the reference panics; a degree above the limit names it
        with pytest.raises(ZeroDivisionError):
            div(fid, w([1, 2]), w([0, 0]))
        with pytest.raises(ValueError, match="32"):
            div(fid, w(rand_poly(f, rng, 100)), w(rand_divisor(f, rng, 33)))
    # deg b = 0: a / b[0]; polynomial_division leaves a untrimmed, the long division's loop gives deg a + 1 coefficients
    a = [5, 0, 7, 0]
    inv = pow(9, -1, f.p)
    q, r = api.polynomial_division(fid, w(a), w([9, 0]))
    assert words_to_ints(q) == stored(f, [v * inv for v in a]) and r.shape == (0, 4)
    q, r = api.polynomial_long_division(fid, w(a), w([9, 0]))
    assert words_to_ints(q) == stored(f, [v * inv for v in a[:3]]) and r.shape == (0, 4)


def test_scale_polynomials_against_the_double_loop():
    from plonky_amd import api
    f, rng = F0, random.Random(900)
    polys = [rand_poly(f, rng, 1000) for _ in range(9)]
    alpha = rng.randrange(f.p)
    want = [0] * 1000
    for i in range(1000):  # plonk_util.rs:290-296
        for j in range(9):
            want[i] = (want[i] + polys[j][i] * pow(alpha, j, f.p)) % f.p
    got = api.scale_polynomials(f.field_id, [ints_to_words(stored(f, c)) for c in polys], ints_to_words(stored(f, [alpha]))[0], 1000)
    assert words_to_ints(got) == stored(f, want)


# ---- errors ----
def test_argument_errors():
    import torch
    from plonky_amd import device as dev, lib
    f, rng = F0, random.Random(1000)
    L = lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_a = dev.to_device(ints_to_words(stored(f, rand_poly(f, rng, 100))))
    d_q = torch.zeros((100, 4), dtype=torch.int64, device="cuda")
    d_r = torch.zeros((40, 4), dtype=torch.int64, device="cuda")

    def call(la, b, q_len, q=d_q):
        bw = ints_to_words(stored(f, b))
        return L.plk_poly_division_dev(f.field_id, ctypes.c_void_p(d_a.data_ptr()), la, bw.ctypes.data_as(ctypes.c_void_p), len(b),
                                       ctypes.c_void_p(q.data_ptr()), q_len, ctypes.c_void_p(d_r.data_ptr()), stream)

    assert call(100, [7], 100) == lib.PLK_ERR_INVALID_ARG                              # lb = 1
    assert "32" in L.plk_last_error().decode()
    assert call(100, rand_divisor(f, rng, 33), 100) == lib.PLK_ERR_INVALID_ARG         # k = 33
    assert "32" in L.plk_last_error().decode()
    assert call(100, [1, 2, 0], 100) == lib.PLK_ERR_INVALID_ARG                        # b[lb - 1] = 0
    assert call(3, [1, 2, 3, 1], 100) == lib.PLK_ERR_INVALID_ARG                       # la <= k
    assert call(2, [1, 2, 3, 1], 100) == lib.PLK_ERR_INVALID_ARG
    assert call(100, [1, 2, 1], 97) == lib.PLK_ERR_INVALID_ARG                         # q_len < la - k
    assert call(100, [1, 2, 1], 98, q=d_a) == lib.PLK_ERR_INVALID_ARG                  # d_q == d_a
    assert call(100, [1, 2, 1], 98) == lib.PLK_OK                                      # and the library still works
    torch.cuda.synchronize()
    hq = np.empty((98, 4), dtype=np.uint64)
    aw, bw = ints_to_words([1] * 100), ints_to_words(stored(f, rand_divisor(f, rng, 33)))
    assert L.plk_poly_division(f.field_id, aw.ctypes.data_as(ctypes.c_void_p), 100, bw.ctypes.data_as(ctypes.c_void_p), 34,
                               hq.ctypes.data_as(ctypes.c_void_p), 98, None) == lib.PLK_ERR_INVALID_ARG
    roots = ints_to_words([1] * 33)
    out = np.empty((34, 4), dtype=np.uint64)
    assert L.plk_poly_from_roots(f.field_id, 33, roots.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == lib.PLK_ERR_INVALID_ARG
    assert "32" in L.plk_last_error().decode()


# ---- full size ----
def test_full_size_2_20():
    """a = q0 b + r0 from seeded words, built on Python integers held in numpy object arrays (one pass per divisor coefficient)."""
    import torch
    from plonky_amd import device as dev
    f, k, la = F0, 3, 1 << 20
    rs = np.random.RandomState(20)

    def draw(n):
        raw = rs.bytes(32 * n)
        return np.array([int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)], dtype=object) % f.p

    def to_words(vals):  # canonical values (object array) -> stored words
        return ints_to_words(list(vals * R % f.p))

    q0, r0 = draw(la - k), draw(k)
    b = np.append(draw(k), 1)
    a = np.zeros(la, dtype=object)
    for i in range(k + 1):
        a[i:i + la - k] += q0 * b[i]
    a[:k] += r0
    a %= f.p
    d_a = dev.to_device(to_words(a))
    q, rem = dev.polynomial_division_dev(f.field_id, d_a, to_words(b))
    torch.cuda.synchronize()
    assert np.array_equal(dev.to_host(q), to_words(q0))
    assert np.array_equal(dev.to_host(rem), to_words(r0))


# ---- the prover's composition ----
def test_public_input_quotient_dev():
    import torch
    from plonky_amd import device as dev
    f, rng, n = F0, random.Random(1200), 1 << 12
    g = f.primitive_root_of_unity(12)
    roots = [pow(g, 5, f.p), pow(g, 4000, f.p)]
    denom = ref_from_roots(f, roots)
    wires = [ref_mul(f, rand_poly(f, rng, n - 2), denom) for _ in range(9)]  # 9 polynomials of 2^12 coefficients that vanish at both points
    alpha = rng.randrange(f.p)
    scaled = [sum(wires[j][i] * pow(alpha, j, f.p) for j in range(9)) % f.p for i in range(n)]
    d_wires = [dev.to_device(ints_to_words(stored(f, c))) for c in wires]
    q, rem = dev.public_input_quotient_dev(f.field_id, d_wires, ints_to_words(stored(f, [alpha]))[0], ints_to_words(stored(f, roots)), n)
    torch.cuda.synchronize()
    assert q.shape == (n, 4) and rem.shape == (2, 4)
    assert words_to_ints(dev.to_host(rem)) == [0, 0]
    qi = canonical(f, words_to_ints(dev.to_host(q)))
    assert qi[n - 2:] == [0, 0]
    assert ref_mul(f, qi[:n - 2], denom) == scaled


# ---- the checked build ----
def run_checked_case():
    rng = random.Random(1300)
    check_division(F0, rand_poly(F0, rng, SHAPE), rand_divisor(F0, rng, 5, 3))
    return 1


CHECKED_BODY = '''
from plonky_amd import device as dev
dev.init()
from tests.test_gpu_poly_division import run_checked_case
print("CHECKED compared", run_checked_case())
'''


def test_checked_build_divides():
    assert "CHECKED compared 1" in checked_child.run_checked(CHECKED_BODY)
