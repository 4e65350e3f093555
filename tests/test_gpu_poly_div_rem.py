"""GPU tests of the series inverse and the division by a divisor of any degree (polydiv_newton.hip): plk_poly_inv_mod_xn[_dev],
plk_poly_div_rem[_dev], api.polynomial_inv_mod_xn / polynomial_div_rem and device.polynomial_inv_mod_xn_dev / polynomial_div_rem_dev.
The field is exact and inverse, quotient and remainder are unique: every comparison is bit for bit on stored words, against
tests/poly_newton_ref.py (schoolbook division and the triangular recurrence on Python integers).

S = 64 is the seed length (PINV_SEED, polyinv_step.cuh): an inverse mod X^m with m <= S runs no Newton level, S < m <= 2 S one, and a
level whose target is not a power of two is truncated."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from tests import checked_child
from tests import poly_newton_ref as nr

FIELDS = [br.TWEEDLEDEE_BASE, br.TWEEDLEDUM_BASE, br.BLS12_377_SCALAR, br.PALLAS_BASE, br.VESTA_BASE]
F0 = br.TWEEDLEDUM_BASE  # Tweedledee's scalar field
S = 64
KS = [1, 2, 32, 33, 64, 65, 255, 1000]
MS = [1, 2, 3, S - 1, S, S + 1, 2 * S, 2 * S + 1, 255, 256, 257, 1000]
POISON = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _init():
    from plonky_amd import device as dev
    dev.init()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(f, vals):
    from plonky_amd import device as dev
    return dev.to_device(nr.ints_to_words(nr.stored(f.p, vals)))


def _host(t):
    from plonky_amd import device as dev
    return nr.words_to_ints(dev.to_host(t))


def divide_dev(f, a, b, q_len=None, with_rem=True, expect_status=0):
    """a, b canonical values -> (q, rem) stored words as integers, through plk_poly_div_rem_dev"""
    import torch
    from plonky_amd import lib
    d_a, d_b = _dev(f, a), _dev(f, b)
    k = len(b) - 1
    q_len = len(a) - k if q_len is None else q_len
    q = torch.full((q_len + 3, 4), POISON, dtype=torch.int64, device="cuda")
    rem = torch.full((k + 3, 4), POISON, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib.check(lib.load().plk_poly_div_rem_dev(len(a), f.field_id, _vp(d_a), _vp(d_b), len(b), _vp(q), q_len, _vp(rem) if with_rem else None, _vp(status),
                                              _stream()))
    torch.cuda.synchronize()
    assert int(status.item()) == expect_status
    assert _host(d_a) == nr.stored(f.p, a) and _host(d_b) == nr.stored(f.p, b), "an input was changed"
    assert _host(q[q_len:]) == [POISON * (1 + (1 << 64) + (1 << 128) + (1 << 192))] * 3, "words beyond q_len were written"
    hr = _host(rem)
    assert hr[k:] == [POISON * (1 + (1 << 64) + (1 << 128) + (1 << 192))] * 3, "words beyond the remainder were written"
    return _host(q[:q_len]), hr[:k]


def check_division(f, a, b, q_len=None):
    q, r = nr.divide(f.p, a, b)
    got_q, got_r = divide_dev(f, a, b, q_len)
    pad = (q_len if q_len is not None else len(q)) - len(q)
    assert got_q == nr.stored(f.p, q) + [0] * pad
    assert got_r == nr.stored(f.p, r)


def rand_divisor(f, rng, k, lead=None):
    return nr.rand_poly(f.p, rng, k) + [rng.randrange(1, f.p) if lead is None else lead]


# ---- the division grid ----
@pytest.mark.parametrize("k", KS)
def test_division_grid(k):
    """no Newton level, one level, a truncated last level; k > m (the divisor longer than the quotient), k >> m, and k = 33, the first
    degree the recurrence route refuses.  Pairs with m k > 2^18 are left out: the schoolbook reference stays under a second."""
    rng = random.Random(100 + k)
    for m in MS:
        if m * k > 1 << 18:
            continue
        check_division(F0, nr.rand_poly(F0.p, rng, k + m), rand_divisor(F0, rng, k, 1 if m % 2 else None))


@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_every_field(f):
    rng = random.Random(200 + f.field_id)
    for k in (33, 65):
        for m in (1, S + 1, 257):
            check_division(f, nr.rand_poly(f.p, rng, k + m), rand_divisor(f, rng, k))


def test_special_inputs():
    f, rng, k, m = F0, random.Random(300), 65, 257
    p = f.p
    b = rand_divisor(f, rng, k)
    q0 = nr.rand_poly(p, rng, m)
    exact = nr.mul_trunc(p, q0, b, k + m)
    q, r = divide_dev(f, exact, b)                                            # a = q0 b: the remainder is all zero
    assert q == nr.stored(p, q0) and r == [0] * k
    check_division(f, nr.rand_poly(p, rng, k + m - 5) + [0] * 5, b)           # q has leading zeros
    a = nr.rand_poly(p, rng, k + m)
    q, r = divide_dev(f, a, [0] * k + [1])                                    # b = X^k: q is a shift, r the low k coefficients
    assert q == nr.stored(p, a[k:]) and r == nr.stored(p, a[:k])
    check_division(f, a, [0] + rand_divisor(f, rng, k - 1))                   # b[0] = 0
    check_division(f, a, rand_divisor(f, rng, k, p - 1))                      # b[k] = p - 1: not monic
    check_division(f, [p - 1] * (k + m), [p - 1] * (k + 1))                   # every coefficient p - 1
    q, r = divide_dev(f, [0] * (k + m), b)                                    # a = 0
    assert q == [0] * m and r == [0] * k
    check_division(f, a, b, q_len=m + 9)                                      # the zero fill
    want_q, _ = nr.divide(p, a, b)
    q, r = divide_dev(f, a, b, with_rem=False)                                # d_rem = NULL: nothing is written there
    assert q == nr.stored(p, want_q) and r == [POISON * (1 + (1 << 64) + (1 << 128) + (1 << 192))] * k


@pytest.mark.parametrize("k", [1, 5, 32])
def test_two_routes_one_answer(k):
    import torch
    from plonky_amd import device as dev, lib
    f, rng, la = F0, random.Random(400 + k), 519
    a, b = nr.rand_poly(f.p, rng, la), rand_divisor(f, rng, k, 1 if k == 5 else None)
    aw, bw = nr.ints_to_words(nr.stored(f.p, a)), nr.ints_to_words(nr.stored(f.p, b))
    q1, r1 = dev.polynomial_division_dev(f.field_id, dev.to_device(aw), bw)
    q2, r2 = dev.polynomial_div_rem_dev(f.field_id, dev.to_device(aw), dev.to_device(bw))
    torch.cuda.synchronize()
    hq, hr = np.empty((la - k, 4), dtype=np.uint64), np.empty((k, 4), dtype=np.uint64)
    lib.check(lib.load().plk_poly_div_rem(la, f.field_id, aw.ctypes.data_as(ctypes.c_void_p), bw.ctypes.data_as(ctypes.c_void_p), k + 1,
                                          hq.ctypes.data_as(ctypes.c_void_p), la - k, hr.ctypes.data_as(ctypes.c_void_p)))
    assert np.array_equal(dev.to_host(q1), dev.to_host(q2)) and np.array_equal(dev.to_host(r1), dev.to_host(r2))
    assert np.array_equal(hq, dev.to_host(q1)) and np.array_equal(hr, dev.to_host(r1))
    want_q, want_r = nr.divide(f.p, a, b)
    assert nr.words_to_ints(hq) == nr.stored(f.p, want_q) and nr.words_to_ints(hr) == nr.stored(f.p, want_r)


def test_host_form_above_the_recurrence_limit():
    from plonky_amd import lib
    f, rng, k, m = F0, random.Random(450), 40, 100
    a, b = nr.rand_poly(f.p, rng, k + m), rand_divisor(f, rng, k)
    aw, bw = nr.ints_to_words(nr.stored(f.p, a)), nr.ints_to_words(nr.stored(f.p, b))
    want_q, want_r = nr.divide(f.p, a, b)
    for with_rem in (True, False):
        hq, hr = np.empty((m + 2, 4), dtype=np.uint64), np.empty((k, 4), dtype=np.uint64)
        lib.check(lib.load().plk_poly_div_rem(k + m, f.field_id, aw.ctypes.data_as(ctypes.c_void_p), bw.ctypes.data_as(ctypes.c_void_p), k + 1,
                                              hq.ctypes.data_as(ctypes.c_void_p), m + 2, hr.ctypes.data_as(ctypes.c_void_p) if with_rem else None))
        assert nr.words_to_ints(hq) == nr.stored(f.p, want_q) + [0, 0]
        if with_rem:
            assert nr.words_to_ints(hr) == nr.stored(f.p, want_r)


# ---- the series inverse ----
@pytest.mark.parametrize("n", [1, 2, 3, S - 1, S, S + 1, 256, 257, 1000])
def test_series_inverse(n):
    """lh < n, = n and > n; in the last case the surplus is poisoned with random words and must not matter"""
    import torch
    from plonky_amd import device as dev
    f, rng = F0, random.Random(500 + n)
    p = f.p
    for lh in sorted({max(1, n // 3), n, n + 7}):
        h = [rng.randrange(1, p)] + nr.rand_poly(p, rng, lh - 1)
        want = nr.inverse_series(p, h[:n], n)
        assert nr.mul_trunc(p, want, h, n) == [1] + [0] * (n - 1)
        words = nr.ints_to_words(nr.stored(p, h))
        if lh > n:
            words[n:] = np.frombuffer(rng.randbytes(32 * (lh - n)), dtype=np.uint64).reshape(-1, 4)  # not even reduced
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        g = dev.polynomial_inv_mod_xn_dev(f.field_id, dev.to_device(words), n, status=status)
        torch.cuda.synchronize()
        got = _host(g)
        assert int(status.item()) == 0 and all(w < p for w in got)
        assert nr.mul_trunc(p, nr.canonical(p, got), h[:n], n) == [1] + [0] * (n - 1)
        assert got == nr.stored(p, want)


@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_series_inverse_every_field(f):
    from plonky_amd import api
    rng, n = random.Random(600 + f.field_id), 2 * S + 3
    h = [f.p - 1] + nr.rand_poly(f.p, rng, n - 1)
    got = api.polynomial_inv_mod_xn(f.field_id, nr.ints_to_words(nr.stored(f.p, h)), n)
    assert nr.words_to_ints(got) == nr.stored(f.p, nr.inverse_series(f.p, h, n))


# ---- larger ----
@pytest.mark.parametrize("la,k", [((1 << 18) + 3, (1 << 9) + 1), ((1 << 16) + 3, (1 << 15) + 1)])
def test_larger(la, k):
    """Schoolbook is too slow here.  Checked: every word below p, the lengths, and a(x) = q(x) b(x) + rem(x) at two seeded random x by
    Horner on Python integers.  Quotient and remainder of degree below la - k and k are unique, and a wrong pair makes
    a - q b - rem a non-zero polynomial of degree below la with at most la roots: it passes one point with probability at most
    la / p < 2^-230."""
    import torch
    from plonky_amd import device as dev
    f, rs = F0, np.random.RandomState(la % 1000 + k)
    p = f.p

    def draw(n):
        raw = rs.bytes(32 * n)
        return [int.from_bytes(raw[32 * i:32 * i + 32], "little") % p for i in range(n)]

    a, b = draw(la), draw(k + 1)
    b[k] = b[k] or 1
    d_a, d_b = dev.to_device(nr.ints_to_words(a)), dev.to_device(nr.ints_to_words(b))  # the draws ARE the stored words
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    q, rem = dev.polynomial_div_rem_dev(f.field_id, d_a, d_b, status=status)
    torch.cuda.synchronize()
    q, rem = _host(q), _host(rem)
    assert int(status.item()) == 0
    assert len(q) == la - k and len(rem) == k
    assert all(w < p for w in q) and all(w < p for w in rem)
    ca, cb, cq, cr = (nr.canonical(p, v) for v in (a, b, q, rem))
    rng = random.Random(la)
    for _ in range(2):
        x = rng.randrange(p)
        assert nr.horner(p, ca, x) == (nr.horner(p, cq, x) * nr.horner(p, cb, x) + nr.horner(p, cr, x)) % p


# ---- status and refusals ----
def test_status_words():
    import torch
    from plonky_amd import device as dev, lib
    f, rng = F0, random.Random(700)
    L = lib.load()
    for n in (5, S + 9):                                                        # h[0] == 0: bit 0, the call returns 0
        h = _dev(f, [0] + nr.rand_poly(f.p, rng, n - 1))
        status = torch.tensor([8], dtype=torch.int32, device="cuda")            # OR-ed into what the caller put there
        dev.polynomial_inv_mod_xn_dev(f.field_id, h, n, status=status)
        torch.cuda.synchronize()
        assert int(status.item()) == 8 | 1
        out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        assert L.plk_poly_inv_mod_xn_dev(n, f.field_id, _vp(h), n, _vp(out), None, _stream()) == lib.PLK_OK   # d_status = NULL
    for k, m in ((3, 5), (70, S + 9)):                                          # b[k] == 0: bit 1
        a, b = nr.rand_poly(f.p, rng, k + m), nr.rand_poly(f.p, rng, k) + [0]
        divide_dev(f, a, b, expect_status=2)
        d_a, d_b = _dev(f, a), _dev(f, b)
        q = torch.zeros((m, 4), dtype=torch.int64, device="cuda")
        assert L.plk_poly_div_rem_dev(k + m, f.field_id, _vp(d_a), _vp(d_b), k + 1, _vp(q), m, None, None, _stream()) == lib.PLK_OK
    torch.cuda.synchronize()
    check_division(f, nr.rand_poly(f.p, rng, 300), rand_divisor(f, rng, 40))    # and the library still works


def test_refusals_launch_nothing():
    import torch
    from plonky_amd import device as dev, lib
    f, rng = F0, random.Random(800)
    L = lib.load()
    INV = lib.PLK_ERR_INVALID_ARG
    a, b = nr.rand_poly(f.p, rng, 100), rand_divisor(f, rng, 40)
    d_a, d_b = _dev(f, a), _dev(f, b)
    d_q = torch.full((100, 4), POISON, dtype=torch.int64, device="cuda")
    d_r = torch.full((100, 4), POISON, dtype=torch.int64, device="cuda")

    def div(la=100, field=f.field_id, pa=d_a, pb=d_b, lb=41, q=d_q, q_len=60, r=d_r):
        return L.plk_poly_div_rem_dev(la, field, _vp(pa), _vp(pb), lb, _vp(q), q_len, _vp(r), None, _stream())

    def inv(n=50, field=f.field_id, h=d_a, lh=100, out=d_q):
        return L.plk_poly_inv_mod_xn_dev(n, field, _vp(h), lh, _vp(out), None, _stream())

    assert div(la=40) == INV and div(la=41, r=None) == lib.PLK_OK               # la <= k; la = k + 1 is the smallest division
    assert div(lb=1) == INV                                                     # lb = 1
    assert div(q_len=59) == INV                                                 # q_len < la - k
    assert inv(n=0) == INV and inv(lh=0) == INV
    for kw in (dict(q=d_a), dict(q=d_b), dict(r=d_a), dict(r=d_b), dict(r=d_q), dict(q=d_a[50:]), dict(r=d_b[40:])):   # every overlap
        assert div(**kw) == INV, kw
    d_h = _dev(f, [5] + a[1:])
    assert inv(out=d_a) == INV and inv(out=d_a[49:]) == INV
    assert inv(h=d_h, out=d_h[50:]) == lib.PLK_OK                               # h is read up to min(lh, n) only
    for bad in (-1, 3, 6, 1000):                                                # the 6-limb field and unknown ids
        for call in (div, inv):
            assert call(field=bad) == INV
            assert L.plk_last_error().decode() == "field %d is not a 4-limb field" % bad
    # a transform beyond the library's largest (2^30) or the field's 2-adicity: refused before anything is touched
    assert inv(n=(1 << 29) + 1) == INV and "transform" in L.plk_last_error().decode()
    assert div(la=(1 << 29) + 42, q_len=(1 << 29) + 2) == INV and "transform" in L.plk_last_error().decode()
    # the host-pointer forms refuse what the device forms report in the status word
    hw = nr.ints_to_words(nr.stored(f.p, [0, 1, 2]))
    out = np.empty((3, 4), dtype=np.uint64)
    assert L.plk_poly_inv_mod_xn(3, f.field_id, hw.ctypes.data_as(ctypes.c_void_p), 3, out.ctypes.data_as(ctypes.c_void_p)) == INV
    assert L.plk_last_error().decode().startswith("Inverse doesn't exist")
    aw, bw = nr.ints_to_words(nr.stored(f.p, a)), nr.ints_to_words(nr.stored(f.p, b[:40] + [0]))
    hq = np.empty((60, 4), dtype=np.uint64)
    assert L.plk_poly_div_rem(100, f.field_id, aw.ctypes.data_as(ctypes.c_void_p), bw.ctypes.data_as(ctypes.c_void_p), 41,
                              hq.ctypes.data_as(ctypes.c_void_p), 60, None) == INV
    torch.cuda.synchronize()
    # nothing was launched: the outputs of the refused calls are untouched (the two accepted probes wrote the front of d_q only)
    assert (dev.to_host(d_r) == np.uint64(POISON)).all() and (dev.to_host(d_q[60:]) == np.uint64(POISON)).all()
    assert _host(d_a) == nr.stored(f.p, a) and _host(d_b) == nr.stored(f.p, b)


# ---- asynchrony ----
def test_two_calls_back_to_back_on_one_stream():
    """different shapes, no synchronisation in between: scratch memory released too early would show in the first result"""
    import torch
    from plonky_amd import device as dev
    f, rng = F0, random.Random(900)
    shapes = [(4000, 700), (300, 65), (1500, 1200)]
    ins = [(nr.rand_poly(f.p, rng, la), rand_divisor(f, rng, k)) for la, k in shapes]
    d_ins = [(_dev(f, a), _dev(f, b)) for a, b in ins]
    h = [rng.randrange(1, f.p)] + nr.rand_poly(f.p, rng, 299)
    d_h = _dev(f, h)
    torch.cuda.synchronize()
    outs = [dev.polynomial_div_rem_dev(f.field_id, d_a, d_b) for d_a, d_b in d_ins]
    g = dev.polynomial_inv_mod_xn_dev(f.field_id, d_h, 300)
    torch.cuda.synchronize()
    for (a, b), (q, r) in zip(ins, outs):
        want_q, want_r = nr.divide(f.p, a, b)
        assert _host(q) == nr.stored(f.p, want_q) and _host(r) == nr.stored(f.p, want_r)
    assert _host(g) == nr.stored(f.p, nr.inverse_series(f.p, h, 300))


# ---- the Python layer ----
def test_api_mirrors_in_every_branch():
    from plonky_amd import api
    f, rng = F0, random.Random(1000)
    p, fid = f.p, f.field_id
    w = lambda vals: nr.ints_to_words(nr.stored(p, vals))
    big = rand_divisor(f, rng, 50)
    q, r = api.polynomial_div_rem(fid, w([0, 0, 0]), w(big))                    # zero a -> ([0], empty)
    assert nr.words_to_ints(q) == [0] and r.shape == (0, 4)
    q, r = api.polynomial_div_rem(fid, w([3, 4, 0]), w(big))                    # deg a < deg b -> ([0], a)
    assert nr.words_to_ints(q) == [0] and nr.words_to_ints(r) == nr.stored(p, [3, 4, 0])
    inv9 = pow(9, -1, p)
    q, r = api.polynomial_div_rem(fid, w([5, 0, 7, 0]), w([9, 0]))              # deg b = 0: a / b[0], untrimmed
    assert nr.words_to_ints(q) == nr.stored(p, [v * inv9 for v in [5, 0, 7, 0]]) and r.shape == (0, 4)
    with pytest.raises(ZeroDivisionError):
        api.polynomial_div_rem(fid, w([1, 2]), w([0, 0]))
    for k in (6, 50):                                                           # both routes: q and r trimmed, untrimmed inputs allowed
        a, b = nr.rand_poly(p, rng, 700) + [0, 0], rand_divisor(f, rng, k) + [0]
        eq, er = nr.divide(p, a[:700], b[:k + 1])
        while er and er[-1] == 0:
            er.pop()
        q, r = api.polynomial_div_rem(fid, w(a), w(b))
        assert nr.words_to_ints(q) == nr.stored(p, eq) and nr.words_to_ints(r) == nr.stored(p, er)
        q0 = nr.rand_poly(p, rng, 300)[:-1] + [5]                               # an exact division: the remainder is empty
        q, r = api.polynomial_div_rem(fid, w(nr.mul_trunc(p, q0, b[:k + 1], 300 + k)), w(b))
        assert nr.words_to_ints(q) == nr.stored(p, q0) and r.shape == (0, 4)
    with pytest.raises(ValueError, match="32"):                                 # polynomial_division itself is unchanged
        api.polynomial_division(fid, w(nr.rand_poly(p, rng, 100)), w(big))
    h = [7] + nr.rand_poly(p, rng, 99)
    assert nr.words_to_ints(api.polynomial_inv_mod_xn(fid, w(h), 150)) == nr.stored(p, nr.inverse_series(p, h, 150))
    with pytest.raises(ValueError, match="Inverse doesn't exist"):
        api.polynomial_inv_mod_xn(fid, w([0, 1]), 4)


def test_device_wrappers_with_and_without_outputs():
    import torch
    from plonky_amd import device as dev
    f, rng, k, la = F0, random.Random(1100), 45, 400
    a, b = nr.rand_poly(f.p, rng, la), rand_divisor(f, rng, k)
    want_q, want_r = nr.divide(f.p, a, b)
    d_a, d_b = _dev(f, a), _dev(f, b)
    q, r = dev.polynomial_div_rem_dev(f.field_id, d_a, d_b)
    assert tuple(q.shape) == (la - k, 4) and tuple(r.shape) == (k, 4)
    out = torch.empty((la, 4), dtype=torch.int64, device="cuda")
    rem = torch.empty((k, 4), dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    q2, r2 = dev.polynomial_div_rem_dev(f.field_id, d_a, d_b, out=out, rem=rem, status=status)
    assert q2 is out and r2 is rem
    q3, _ = dev.polynomial_div_rem_dev(f.field_id, d_a, d_b, q_len=la - k + 5)
    torch.cuda.synchronize()
    assert _host(q) == nr.stored(f.p, want_q) and _host(r) == nr.stored(f.p, want_r)
    assert _host(out) == nr.stored(f.p, want_q) + [0] * k and _host(rem) == nr.stored(f.p, want_r) and int(status.item()) == 0
    assert _host(q3) == nr.stored(f.p, want_q) + [0] * 5
    g_out = torch.empty((70, 4), dtype=torch.int64, device="cuda")
    h = [3] + nr.rand_poly(f.p, rng, 20)
    assert dev.polynomial_inv_mod_xn_dev(f.field_id, _dev(f, h), 70, out=g_out) is g_out
    torch.cuda.synchronize()
    assert _host(g_out) == nr.stored(f.p, nr.inverse_series(f.p, h, 70))


# ---- the checked build ----
def run_checked_case():
    from plonky_amd import api
    f, rng = F0, random.Random(1200)
    check_division(f, nr.rand_poly(f.p, rng, 65 + 257), rand_divisor(f, rng, 65))
    h = [rng.randrange(1, f.p)] + nr.rand_poly(f.p, rng, 256)
    assert nr.words_to_ints(api.polynomial_inv_mod_xn(f.field_id, nr.ints_to_words(nr.stored(f.p, h)), 257)) == nr.stored(f.p, nr.inverse_series(f.p, h, 257))
    return 2


CHECKED_BODY = '''
from plonky_amd import device as dev
dev.init()
from tests.test_gpu_poly_div_rem import run_checked_case
print("CHECKED compared", run_checked_case())
'''


def test_checked_build_divides_and_inverts():
    assert "CHECKED compared 2" in checked_child.run_checked(CHECKED_BODY)
