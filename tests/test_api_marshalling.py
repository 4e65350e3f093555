"""CPU-only: what plonky_amd.api hands to the C ABI, pinned from outside.  The library is replaced by the recorder of abi_recorder.py;
every test states the C call it expects literally - the entry point, the arguments and their order - and what comes back: shape and
dtype, the exception type and message of every panic translation and refusal, and what an id outside the tables does (a KeyError
in Python, or a call that reaches the library to be refused there).  libplonky_hip.so is never loaded.

Host limbs are compared by their content read back through the pointer, scalars and sizes by value.  Results that depend on what
the library wrote come from the recorder's replies; nothing is compared that derives from an output nobody wrote."""
import ctypes
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

from plonky_amd import api, lib
from tests.abi_recorder import ANYPTR, H, HA, HND, NULL, OUT, OUTS, P, REF, VA, _Recorder, call, refused

FIELDS = ((0, 4), (3, 6))  # (field id, limbs): TweedledeeBase, Bls12377Base
CURVES = ((0, 4), (2, 6))  # (curve id, limbs): Tweedledee, Bls12377
BAD = 9  # an id outside _FIELD_LIMBS and _CURVE_LIMBS
INVALID, HIP = lib.PLK_ERR_INVALID_ARG, lib.PLK_ERR_HIP
CTX, HANDLE = "ctx", "rescue-handle"
U8 = np.uint8


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(api._lib, "load", lambda: r)
    return r


def limbs(*shape, seed=1):
    return (np.arange(int(np.prod(shape)), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)).reshape(shape)


def flags(n):
    return (np.arange(n) % 2).astype(np.uint8)


def is_u64(a, *shape):
    return isinstance(a, np.ndarray) and a.shape == shape and a.dtype == np.uint64


def raises(rec, exc, message, fn, *args, **kwargs):
    """the wrapper raises exactly this type with exactly this message; returns the entries it called"""
    rec.calls, rec.want = [], []
    with pytest.raises(exc) as e:
        fn(*args, **kwargs)
    assert type(e.value) is exc and (message is None or str(e.value) == message), (type(e.value), str(e.value))
    names = [c[0] for c in rec.calls]
    rec.calls = []
    return names


def untouched(rec, exc, message, fn, *args, **kwargs):
    """a Python-side refusal: nothing reaches the library"""
    assert raises(rec, exc, message, fn, *args, **kwargs) == []


def key_error(rec, fn, *args, **kwargs):
    """an id outside the tables that Python stops"""
    untouched(rec, KeyError, None, fn, *args, **kwargs)


def reaches(rec, entry, fn, *args, **kwargs):
    """an id outside the tables that goes to the library to be refused there: the first call is `entry`, the id in it"""
    rec.calls, rec.want = [], []
    fn(*args, **kwargs)
    assert rec.calls[0][0] == entry and BAD in rec.calls[0][1:4]
    rec.calls = []


def names(rec, fn, *args, **kwargs):
    rec.calls, rec.want = [], []
    result = fn(*args, **kwargs)
    got = [c[0] for c in rec.calls]
    rec.calls = []
    return got, result


def panics(rec, entry, text, exc, message, fn, *args, **kwargs):
    """the library refuses with PLK_ERR_INVALID_ARG and this text -> the wrapper's translation, after that one call"""
    rec.reply(entry, rc=INVALID, error=text)
    assert raises(rec, exc, message, fn, *args, **kwargs) == [entry]


def other_status(rec, entry, fn, *args, **kwargs):
    """any status the wrapper does not translate is PlonkyHipError, with the code and the library's text"""
    for rc, text in ((HIP, "hipErrorUnknown"), (INVALID, "something else")):
        rec.reply(entry, rc=rc, error=text)
        with pytest.raises(lib.PlonkyHipError) as e:
            fn(*args, **kwargs)
        assert e.value.code == rc and str(e.value) == "libplonky_hip error %d: %s" % (rc, text)
    rec.calls = []


def hip_error(rec, entry, fn, *args, **kwargs):
    """the wrappers that turn every PLK_ERR_INVALID_ARG into ValueError: the other codes are PlonkyHipError"""
    rec.reply(entry, rc=HIP, error="hipErrorUnknown")
    raises(rec, lib.PlonkyHipError, "libplonky_hip error %d: hipErrorUnknown" % HIP, fn, *args, **kwargs)


# ---- devices ----
def test_init_devices(rec):
    rec.reply("plk_device_count", rc=3)
    assert call(rec, [("plk_init_devices", 2), ("plk_device_count",)], api.init_devices, 2) == 3
    rec.reply("plk_device_count", rc=5)
    assert call(rec, ("plk_device_count",), api.device_count) == 5
    other_status(rec, "plk_init_devices", api.init_devices)


# ---- transforms ----
def test_fft_precompute(rec):
    for field, _ in FIELDS:
        pre = call(rec, ("plk_ntt_precompute", field, 3), api.fft_precompute, field, 5)
        assert (pre.field, pre.degree_pow, pre.size()) == (field, 3, 8)
    untouched(rec, AssertionError, "n_power <= TWO_ADICITY", api.fft_precompute, 4, (1 << 32) + 1)
    key_error(rec, api.fft_precompute, BAD, 4)
    other_status(rec, "plk_ntt_precompute", api.fft_precompute, 0, 4)


def test_fft_precompute_table(rec):
    for field, L in FIELDS:
        got = call(rec, ("plk_ntt_precompute_table", field, 2, OUT(0)), api.fft_precompute_table, field, 3)
        assert [g.shape for g in got] == [(1, L), (2, L), (4, L)] and all(g.dtype == np.uint64 for g in got)
    untouched(rec, AssertionError, "n_power <= TWO_ADICITY", api.fft_precompute_table, 4, (1 << 32) + 1)
    key_error(rec, api.fft_precompute_table, BAD, 4)


def test_fft_with_precomputation(rec):
    for (field, L), inverse in itertools.product(FIELDS, (False, True)):
        x = limbs(4, L)
        fn = api.ifft_with_precomputation_power_of_2 if inverse else api.fft_with_precomputation_power_of_2
        pre = api.FftPrecomputation(field, 5)  # release builds accept any table at least as large
        assert is_u64(call(rec, ("plk_ntt", field, 2, 1 if inverse else 0, H(x), OUT()), fn, x.tolist(), pre), 4, L)
        refused(rec, fn, limbs(3, L), pre)  # Not a power of two
        assert is_u64(call(rec, ("plk_ntt", field, 2, 0, H(x), OUT()), api.fft_with_precomputation, x, pre), 4, L)
        y = limbs(5, L)
        assert is_u64(call(rec, ("plk_ntt_padded", field, 3, H(y), 5, OUT()), api.fft_with_precomputation, y.reshape(-1), pre), 8, L)
        assert is_u64(call(rec, [("plk_ntt_precompute", field, 3), ("plk_ntt_padded", field, 3, H(y), 5, OUT())], api.fft, field, y), 8, L)
        assert is_u64(call(rec, [("plk_ntt_precompute", field, 2), ("plk_ntt", field, 2, 0, H(x), OUT())], api.fft, field, x), 4, L)
    untouched(rec, AssertionError, "Not a power of two", api.fft_with_precomputation_power_of_2, limbs(3, 4), api.FftPrecomputation(0, 2))
    bad = api.FftPrecomputation(BAD, 2)
    for fn in (api.fft_with_precomputation_power_of_2, api.ifft_with_precomputation_power_of_2, api.fft_with_precomputation):
        key_error(rec, fn, limbs(4, 4), bad)
    key_error(rec, api.fft, BAD, limbs(4, 4))
    other_status(rec, "plk_ntt", api.fft_with_precomputation_power_of_2, limbs(4, 4), api.FftPrecomputation(0, 2))
    other_status(rec, "plk_ntt_padded", api.fft_with_precomputation, limbs(3, 4), api.FftPrecomputation(0, 2))


def test_fft_batch_and_values_to_polynomials(rec):
    for field, inverse in itertools.product((0, 1), (False, True)):
        polys = limbs(3, 4, 4)
        got = call(rec, ("plk_ntt_batch", field, 2, 1 if inverse else 0, 3, HA(polys), OUTS()), api.fft_batch, field, polys.tolist(), inverse=inverse)
        assert is_u64(got, 3, 4, 4)
    got = call(rec, ("plk_ntt_batch", 0, 2, 1, 3, HA(polys), OUTS()), api.values_to_polynomials, polys, api.FftPrecomputation(0, 2))
    assert is_u64(got, 3, 4, 4)
    refused(rec, api.fft_batch, 0, limbs(2, 3, 4))
    reaches(rec, "plk_ntt_batch", api.fft_batch, BAD, limbs(2, 4, 4))
    other_status(rec, "plk_ntt_batch", api.fft_batch, 0, limbs(2, 4, 4))


def test_polynomials_to_values_padded(rec):
    pre = api.FftPrecomputation(0, 4)
    ps = [limbs(2, 4), limbs(1, 4, seed=3)]
    got = call(rec, ("plk_ntt_padded_batch", 0, 4, 2, HA(ps), VA([2, 1]), OUTS()), api.polynomials_to_values_padded, [p.tolist() for p in ps], pre)
    assert is_u64(got, 2, 16, 4)
    got, result = names(rec, api.polynomials_to_values_padded, [], pre)
    assert got == [] and is_u64(result, 0, 16, 4)
    untouched(rec, AssertionError, "fft.rs:107-111: the table is too small for the padded polynomial", api.polynomials_to_values_padded, [limbs(3, 4)], pre)
    key_error(rec, api.polynomials_to_values_padded, ps, api.FftPrecomputation(BAD, 4))
    other_status(rec, "plk_ntt_padded_batch", api.polynomials_to_values_padded, ps, pre)


# ---- polynomial callers of the NTT ----
def test_polynomial_divide_by_z_h(rec):
    for (field, L), (length, cap, out_len) in itertools.product(FIELDS, ((5, 8, 4), (8, 8, 8), (1, 1, 0))):
        x = limbs(length, L)
        rec.reply("plk_poly_divide_by_z_h", write={6: out_len})
        got = call(rec, ("plk_poly_divide_by_z_h", field, H(x), length, 2, ANYPTR, cap, REF(ctypes.c_size_t)), api.polynomial_divide_by_z_h, field, x, 2)
        assert is_u64(got, out_len, L) and not got.any() and got.base is None  # a copy of the zeroed buffer's head
    refused(rec, api.polynomial_divide_by_z_h, 0, limbs(5, 4), 0)
    key_error(rec, api.polynomial_divide_by_z_h, BAD, limbs(5, 4), 2)
    other_status(rec, "plk_poly_divide_by_z_h", api.polynomial_divide_by_z_h, 0, limbs(5, 4), 2)


def test_polynomial_mul(rec):
    for field, L in FIELDS:
        a, b = limbs(3, L), limbs(2, L, seed=5)
        rec.reply("plk_poly_mul", write={7: 4})
        got = call(rec, ("plk_poly_mul", field, H(a), 3, H(b), 2, ANYPTR, 8, REF(ctypes.c_size_t)), api.polynomial_mul, field, a, b.tolist())
        assert is_u64(got, 4, L) and not got.any() and got.base is None
    assert is_u64(call(rec, ("plk_poly_mul", 0, H(a[:0]), 0, H(a[:0]), 0, ANYPTR, 1, REF(ctypes.c_size_t)), api.polynomial_mul, 0, [], []), 0, 4)
    key_error(rec, api.polynomial_mul, BAD, limbs(3, 4), limbs(2, 4))
    other_status(rec, "plk_poly_mul", api.polynomial_mul, 0, limbs(3, 4), limbs(2, 4))


def _poly(*coeffs):
    """a (len, 4) polynomial with these small coefficients"""
    x = np.zeros((len(coeffs), 4), dtype=np.uint64)
    x[:, 0] = coeffs
    return x


def test_polynomial_division_branches(rec):
    a, b = _poly(1, 2, 3, 4, 0), _poly(5, 6, 7, 0)  # degree_plus_one 4 and 3: the trailing zero rows are not sent
    for fn in (api.polynomial_division, api.polynomial_long_division):
        q, r = call(rec, ("plk_poly_division", 0, H(a[:4]), 4, H(b[:3]), 3, OUT(0), 2, ANYPTR), fn, 0, a, b.tolist())
        assert is_u64(q, 2, 4) and r.dtype == np.uint64 and r.shape[1:] == (4,) and r.shape[0] <= 2
    q, r = call(rec, ("plk_poly_div_rem", 4, 0, H(a[:4]), H(b[:3]), 3, OUT(0), 2, ANYPTR), api.polynomial_div_rem, 0, a, b)
    assert is_u64(q, 2, 4) and r.dtype == np.uint64 and r.shape[1:] == (4,) and r.shape[0] <= 2
    for fn in (api.polynomial_division, api.polynomial_div_rem, api.polynomial_long_division):
        untouched(rec, ZeroDivisionError, "Division by zero polynomial", fn, 0, a, _poly(0, 0))
        got, (q, r) = names(rec, fn, 0, _poly(0, 0), b)  # a zero a
        assert got == [] and is_u64(q, 1, 4) and not q.any() and is_u64(r, 0, 4)
        got, (q, r) = names(rec, fn, 0, b, a)  # deg a < deg b
        assert got == [] and is_u64(q, 1, 4) and not q.any() and np.array_equal(r, b)
        key_error(rec, fn, BAD, a, b)
    # a constant divisor: a / b[0], one inverse and one product, untrimmed; polynomial_long_division trims a first
    for fn, rows in ((api.polynomial_division, 5), (api.polynomial_div_rem, 5), (api.polynomial_long_division, 4)):
        got, (q, r) = names(rec, fn, 0, a, _poly(7, 0))
        assert got == ["plk_field_op", "plk_field_op"] and is_u64(q, rows, 4) and is_u64(r, 0, 4)
    big = np.ones((40, 4), dtype=np.uint64)
    untouched(rec, ValueError, "divisor of degree 33: at most 32 (PLK_POLY_DIV_MAX_DEGREE)", api.polynomial_division, 0, big, big[:34])
    assert names(rec, api.polynomial_division, 0, big, big[:33])[0] == ["plk_poly_division"]
    assert names(rec, api.polynomial_div_rem, 0, big, big[:34])[0] == ["plk_poly_div_rem"]
    other_status(rec, "plk_poly_division", api.polynomial_division, 0, a, b)
    other_status(rec, "plk_poly_div_rem", api.polynomial_div_rem, 0, a, b)


def test_polynomial_inv_mod_xn(rec):
    for field, L in FIELDS:
        h = limbs(3, L)
        assert is_u64(call(rec, ("plk_poly_inv_mod_xn", 5, field, H(h), 3, OUT()), api.polynomial_inv_mod_xn, field, h.tolist(), 5), 5, 4)  # (n, 4) whatever L
    untouched(rec, ValueError, "Inverse doesn't exist.", api.polynomial_inv_mod_xn, 0, _poly(0, 1), 5)
    refused(rec, api.polynomial_inv_mod_xn, 0, limbs(3, 4), 0)
    refused(rec, api.polynomial_inv_mod_xn, 0, limbs(0, 4), 2)
    key_error(rec, api.polynomial_inv_mod_xn, BAD, limbs(3, 4), 5)
    other_status(rec, "plk_poly_inv_mod_xn", api.polynomial_inv_mod_xn, 0, limbs(3, 4), 5)


def test_polynomial_from_roots(rec):
    r = limbs(3, 4)
    assert is_u64(call(rec, ("plk_poly_from_roots", 1, 3, H(r), OUT()), api.polynomial_from_roots, 1, r.reshape(-1).tolist()), 4, 4)
    reaches(rec, "plk_poly_from_roots", api.polynomial_from_roots, BAD, r)
    other_status(rec, "plk_poly_from_roots", api.polynomial_from_roots, 0, r)


# ---- the MSM ----
def _pre(curve, n):
    return SimpleNamespace(_ctx=CTX, n=n, curve=curve)


def test_msm_precompute_and_the_context(rec):
    for (curve, L), n in itertools.product(CURVES, (1, 3)):
        g, z = limbs(n, 2, L), flags(n)
        rec.reply("plk_msm_precompute_ex", write={6: 0xC0FFEE})
        pre = call(rec, ("plk_msm_precompute_ex", curve, n, H(g), NULL, 0, 0, REF(ctypes.c_void_p)), api.msm_precompute, curve, g.tolist(), 7)
        assert (pre.curve, pre.n, pre.w, len(pre)) == (curve, n, 7, n) and isinstance(pre._ctx, ctypes.c_void_p) and pre._ctx.value == 0xC0FFEE
        rec.reply("plk_msm_ctx_window", rc=13)
        assert call(rec, ("plk_msm_ctx_window", HND(0xC0FFEE)), lambda: pre.window) == 13
        rec.reply("plk_msm_free", rc=HIP)  # the status of plk_msm_free is not looked at
        call(rec, ("plk_msm_free", HND(0xC0FFEE)), pre.free)
        assert pre._ctx is None and names(rec, pre.free)[0] == []
        pre = call(rec, ("plk_msm_precompute_ex", curve, n, H(g), H(z, U8), 13, 1, REF(ctypes.c_void_p)), api.msm_precompute, curve, g, 8, zero=z.tolist(),
                   device_window=13, table_free=True)
        assert names(rec, pre.free)[0] == []  # a context the library never handed out is not freed
    refused(rec, api.msm_precompute, 0, limbs(3, 2, 4), 8, zero=flags(2))
    key_error(rec, api.msm_precompute, BAD, limbs(3, 2, 4), 8)
    other_status(rec, "plk_msm_precompute_ex", api.msm_precompute, 0, limbs(3, 2, 4), 8)


def test_msm_execute(rec):
    assert api.msm_execute is api.msm_execute_parallel
    for (curve, L), n in itertools.product(CURVES, (0, 3)):
        s = limbs(n, 4)
        xy, z = call(rec, ("plk_msm_execute", CTX, H(s), n, OUT(0), ANYPTR), api.msm_execute_parallel, _pre(curve, n), s.tolist())
        assert is_u64(xy, 2, L) and not xy.any() and z == 0 and type(z) is int
        xy, z = call(rec, ("plk_msm_execute_projective", CTX, H(s), n, OUT(0), ANYPTR), api.msm_execute_parallel_projective, _pre(curve, n), s)
        assert is_u64(xy, 3, L) and not xy.any() and z == 0 and type(z) is int
        sv = limbs(2, n, 4)
        xy, z = call(rec, ("plk_msm_execute_batch", CTX, 2, HA(sv), n, OUT(0), OUT(1)), api.msm_execute_batch, _pre(curve, n), sv.reshape(2, -1))
        assert is_u64(xy, 2, 2, L) and not xy.any() and z.shape == (2,) and z.dtype == U8 and not z.any()
    message = "powers_per_generator.len() != scalars.len()"
    for fn in (api.msm_execute_parallel, api.msm_execute_parallel_projective):
        untouched(rec, AssertionError, message, fn, _pre(0, 3), limbs(2, 4))
        key_error(rec, fn, _pre(BAD, 3), limbs(3, 4))
    untouched(rec, AssertionError, message, api.msm_execute_batch, _pre(0, 3), limbs(2, 2, 4))
    key_error(rec, api.msm_execute_batch, _pre(BAD, 3), limbs(2, 3, 4))
    other_status(rec, "plk_msm_execute", api.msm_execute_parallel, _pre(0, 3), limbs(3, 4))
    other_status(rec, "plk_msm_execute_projective", api.msm_execute_parallel_projective, _pre(0, 3), limbs(3, 4))
    other_status(rec, "plk_msm_execute_batch", api.msm_execute_batch, _pre(0, 3), limbs(2, 3, 4))


def test_msm_parallel(rec):
    for curve, L in CURVES:
        g, s, z = limbs(3, 2, L), limbs(3, 4, seed=9), flags(3)
        rec.reply("plk_msm_precompute_ex", write={6: 0xBEEF})
        xy, oz = call(rec, [("plk_msm_precompute_ex", curve, 3, H(g), H(z, U8), 0, 1, REF(ctypes.c_void_p)),
                            ("plk_msm_execute", HND(0xBEEF), H(s), 3, OUT(0), ANYPTR), ("plk_msm_free", HND(0xBEEF))], api.msm_parallel, curve, s, g, 4, zero=z)
        assert is_u64(xy, 2, L) and oz == 0
    rec.reply("plk_msm_precompute_ex", write={6: 0xBEEF})
    rec.reply("plk_msm_execute", rc=HIP, error="hipErrorUnknown")  # the context is freed on the way out
    assert raises(rec, lib.PlonkyHipError, None, api.msm_parallel, 0, limbs(3, 4), limbs(3, 2, 4), 4) == ["plk_msm_precompute_ex", "plk_msm_execute", "plk_msm_free"]
    key_error(rec, api.msm_parallel, BAD, limbs(3, 4), limbs(3, 2, 4), 4)


def test_commitment_precompute_and_coeffs_vec_to_commitments(rec):
    for curve, L in CURVES:
        g, h = limbs(3, 2, L), limbs(1, 2, L, seed=5)
        pre = call(rec, ("plk_msm_precompute_ex", curve, 4, H(np.concatenate([g, h])), NULL, 11, 0, REF(ctypes.c_void_p)), api.commitment_precompute, curve, g,
                   h.reshape(2, L), 8, device_window=11)
        assert (pre.n, pre.w) == (4, 8)
        cv, r = limbs(2, 3, 4), limbs(2, 4, seed=7)
        rows = np.concatenate([cv, r.reshape(2, 1, 4)], axis=1)
        xy, z = call(rec, ("plk_msm_execute_batch", CTX, 2, HA(rows), 4, OUT(0), OUT(1)), api.coeffs_vec_to_commitments, _pre(curve, 4), cv, r)
        assert is_u64(xy, 2, 2, L) and z.shape == (2,) and z.dtype == U8
    refused(rec, api.commitment_precompute, 0, limbs(3, 2, 4), limbs(2, 2, 4), 8)
    untouched(rec, AssertionError, "coefficients.len() must equal the number of generators (curve_msm.rs:106)", api.coeffs_vec_to_commitments, _pre(0, 4),
              limbs(2, 4, 4), limbs(2, 4))
    key_error(rec, api.commitment_precompute, BAD, limbs(3, 2, 4), limbs(1, 2, 4), 8)


def test_msm_precompute_table(rec):
    for (curve, L), zero in itertools.product(CURVES, (None, flags(2))):
        g = limbs(2, 2, L)
        rec.reply("plk_msm_table_digits", rc=3)
        zp = NULL if zero is None else H(zero, U8)
        t, tz = call(rec, [("plk_msm_table_digits", curve, 5), ("plk_msm_precompute_table", curve, 2, H(g), zp, 5, OUT(0), OUT(1))], api.msm_precompute_table,
                     curve, g, 5, zero=zero)
        assert is_u64(t, 2, 3, 2, L) and not t.any() and tz.shape == (2, 3) and tz.dtype == U8 and not tz.any()
    assert raises(rec, AssertionError, "", api.msm_precompute_table, 0, limbs(2, 2, 4), 5) == ["plk_msm_table_digits"]  # no digits: refused after the question
    key_error(rec, api.msm_precompute_table, BAD, limbs(2, 2, 4), 5)
    rec.reply("plk_msm_table_digits", rc=3)
    rec.reply("plk_msm_precompute_table", rc=HIP, error="hipErrorUnknown")
    raises(rec, lib.PlonkyHipError, "libplonky_hip error %d: hipErrorUnknown" % HIP, api.msm_precompute_table, 0, limbs(2, 2, 4), 5)


def test_msm_debug_digits(rec):
    s = limbs(2, 4)
    rec.reply("plk_msm_debug_digits", write={5: 3})
    d, unsigned, carry = call(rec, [("plk_msm_debug_digits", 2, 7, 0, NULL, NULL, REF(ctypes.c_uint)),
                                    ("plk_msm_debug_digits", 2, 7, 2, H(s), OUT(0), REF(ctypes.c_uint))], api.msm_debug_digits, 2, s.tolist(), 7)
    assert d.shape == (2, 3) and d.dtype == np.int32 and unsigned.shape == (2, 3) and unsigned.dtype == np.int64 and carry.shape == (2,) and carry.dtype == np.int64
    assert not d.any() and not unsigned.any() and not carry.any()
    reaches(rec, "plk_msm_debug_digits", api.msm_debug_digits, BAD, s, 7)
    other_status(rec, "plk_msm_debug_digits", api.msm_debug_digits, 0, s, 7)


# ---- points ----
def test_fold_generators(rec):
    sl, sh = limbs(4, seed=2), limbs(4, seed=3)
    for (curve, L), m, with_flags in itertools.product(CURVES, (1, 2), (False, True)):
        lo, hi = limbs(m, 2, L), limbs(m, 2, L, seed=5)
        lz, hz = (flags(m), 1 - flags(m)) if with_flags else (None, None)
        out, oz = call(rec, ("plk_curve_fold_pairs", curve, m, H(lo), H(lz, U8) if with_flags else NULL, H(hi), H(hz, U8) if with_flags else NULL, H(sl), H(sh),
                             OUT(0), OUT(1)), api.fold_generators, curve, lo, hi.tolist(), sl.tolist(), sh.reshape(1, 4), lo_zero=lz, hi_zero=hz)
        assert is_u64(out, m, 2, L) and not out.any() and oz.shape == (m,) and oz.dtype == U8
    refused(rec, api.fold_generators, 0, limbs(2, 2, 4), limbs(3, 2, 4), sl, sh)
    key_error(rec, api.fold_generators, BAD, limbs(2, 2, 4), limbs(2, 2, 4), sl, sh)
    other_status(rec, "plk_curve_fold_pairs", api.fold_generators, 0, limbs(2, 2, 4), limbs(2, 2, 4), sl, sh)


def test_curve_sums(rec):
    for (curve, L), zero in itertools.product(CURVES, (None, flags(3))):
        p = limbs(3, 2, L)
        zp = NULL if zero is None else H(zero, U8)
        for fn in (api.curve_sum_affine, api.affine_summation_best):
            out, z = call(rec, ("plk_curve_sum_affine", curve, 3, H(p), zp, OUT(0), ANYPTR), fn, curve, p.tolist(), zero)
            assert is_u64(out, 2, L) and not out.any() and z == 0 and type(z) is int
        q = limbs(1, 2, L, seed=4)
        got = call(rec, [("plk_curve_sum_affine", curve, 3, H(p), zp, ANYPTR, ANYPTR), ("plk_curve_sum_affine", curve, 1, H(q), NULL if zero is None else H([1], U8),
                                                                                        ANYPTR, ANYPTR)],
                   api.affine_multisummation_best, curve, [p, q.tolist()], None if zero is None else [zero, [1]])
        assert len(got) == 2 and all(is_u64(o, 2, L) and z == 0 for o, z in got)
    key_error(rec, api.curve_sum_affine, BAD, limbs(3, 2, 4))
    key_error(rec, api.affine_multisummation_best, BAD, [])
    other_status(rec, "plk_curve_sum_affine", api.curve_sum_affine, 0, limbs(3, 2, 4))


def test_batch_to_affine(rec):
    for (curve, L), zero in itertools.product(CURVES, (None, flags(2))):
        p = limbs(2, 3, L)
        out, oz = call(rec, ("plk_curve_batch_to_affine", curve, 2, H(p), NULL if zero is None else H(zero, U8), OUT(0), OUT(1)), api.batch_to_affine, curve,
                       p.reshape(-1), zero)
        assert is_u64(out, 2, 2, L) and oz.shape == (2,) and oz.dtype == U8 and not oz.any()
    key_error(rec, api.batch_to_affine, BAD, limbs(2, 3, 4))
    other_status(rec, "plk_curve_batch_to_affine", api.batch_to_affine, 0, limbs(2, 3, 4))


OPS = ("add", "sub", "mul", "neg", "square", "inverse", "to_canonical", "from_canonical", "inverse_euclid", "inverse_divsteps", "inverse_divsteps_var",
       "inverse_divsteps_one_lane", "mul_add2_edge", "wide_sum", "sqrt", "sqrt_tabled")


def test_field_op(rec):
    assert api.FIELD_OPS == {op: code for code, op in enumerate(OPS)}
    for (field, L), (code, op) in itertools.product(FIELDS, enumerate(OPS)):
        a, b = limbs(3, L), limbs(3, L, seed=7)
        assert is_u64(call(rec, ("plk_field_op", field, code, H(a), H(b), OUT(), 3), api.field_op, field, op, a.tolist(), b.reshape(-1)), 3, L)
    assert is_u64(call(rec, ("plk_field_op", 0, 3, P(a4 := limbs(1, 4)), P(a4), OUT(), 1), api.field_op, 0, "neg", a4), 1, 4)  # b=None: a stands in
    assert is_u64(call(rec, ("plk_field_op", 0, 3, P(a4), P(a4), OUT(), 1), api.field_op, 0, "neg", a4, None), 1, 4)
    key_error(rec, api.field_op, BAD, "add", limbs(1, 4))
    key_error(rec, api.field_op, 0, "no such op", limbs(1, 4))
    other_status(rec, "plk_field_op", api.field_op, 0, "add", limbs(1, 4), limbs(1, 4))


def test_curve_op(rec):
    assert api.CURVE_OPS == {"add": 0, "dbl": 1, "add_q": 2, "dbl_q": 3, "madd": 4, "madd_entry": 5, "dbl_q_times": 6, "wave_sum_q": 7, "chain_q": 8}
    for curve, L in CURVES:
        axy, az, al = limbs(3, 2, L), flags(3), limbs(3, L, seed=3)
        bxy, bz, bl = limbs(3, 2, L, seed=5), 1 - flags(3), limbs(3, L, seed=7)
        out, oz, mism = call(rec, ("plk_curve_op", curve, 0, 0, 3, H(axy), H(az, U8), H(al), H(bxy), H(bz, U8), H(bl), H([0, 0, 0], U8), OUT(0), OUT(1),
                                   REF(ctypes.c_uint)), api.curve_op, curve, "add", (axy.tolist(), az.tolist(), al.reshape(-1)), (bxy, bz, bl))
        assert is_u64(out, 3, 2, L) and not out.any() and oz.shape == (3,) and oz.dtype == U8 and mism == 0xFFFFFFFF and type(mism) is int
        fl = np.array([1, 2, 3], dtype=U8)
        out, oz, mism = call(rec, ("plk_curve_op", curve, 7, 2, 3, H(axy), NULL, H(al), NULL, NULL, NULL, H(fl, U8), OUT(0), OUT(1), REF(ctypes.c_uint)),
                             api.curve_op, curve, "wave_sum_q", (axy, None, al), flags=fl.tolist(), param=2)
        assert is_u64(out, 2, 2, L) and oz.shape == (2,)  # ceil(3 / 2) sums
        call(rec, ("plk_curve_op", curve, 4, 0, 3, H(axy), NULL, H(al), H(bxy), H(bz, U8), NULL, ANYPTR, OUT(0), OUT(1), REF(ctypes.c_uint)),
             api.curve_op, curve, "madd", (axy, None, al), (bxy, bz, None))
        rec.reply("plk_curve_op", write={13: 5})
        assert names(rec, api.curve_op, curve, "dbl", (axy, az, al))[1][2] == 5
    key_error(rec, api.curve_op, BAD, "add", (limbs(3, 2, 4), None, limbs(3, 4)))
    key_error(rec, api.curve_op, 0, "no such op", (limbs(3, 2, 4), None, limbs(3, 4)))
    other_status(rec, "plk_curve_op", api.curve_op, 0, "dbl", (limbs(3, 2, 4), None, limbs(3, 4)))


# ---- the Plonk loops ----
def test_evaluate_all_constraints(rec):
    k, l, r, b = limbs(2, 6, 4), limbs(2, 9, 4, seed=2), limbs(2, 9, 4, seed=3), limbs(2, 9, 4, seed=4)
    zeta, a = limbs(4, seed=5), limbs(4, seed=6)
    got = call(rec, ("plk_plonk_evaluate_all_constraints", 1, 2, H(k), H(l), H(r), H(b), H(zeta), H(a), OUT()), api.evaluate_all_constraints, 1, k.tolist(),
               l.reshape(-1), r, b, zeta.tolist(), a.reshape(1, 4))
    assert is_u64(got, 2, 8, 4)
    refused(rec, api.evaluate_all_constraints, 1, k, l, r[:1], b, zeta, a)
    reaches(rec, "plk_plonk_evaluate_all_constraints", api.evaluate_all_constraints, BAD, k, l, r, b, zeta, a)
    other_status(rec, "plk_plonk_evaluate_all_constraints", api.evaluate_all_constraints, 1, k, l, r, b, zeta, a)


def test_vanishing_points(rec):
    c, w, s, z, ks = limbs(6, 16, 4), limbs(9, 16, 4, seed=2), limbs(6, 16, 4, seed=3), limbs(16, 4, seed=4), limbs(6, 4, seed=5)
    sc = [limbs(4, seed=s_) for s_ in range(6, 11)]
    got = call(rec, ("plk_plonk_vanishing_points", 1, 1, H(c), H(w), H(s), H(z), H(ks), *[H(x) for x in sc], OUT()), api.vanishing_points, 1, 2, c.tolist(),
               w.reshape(-1), s, z, ks.tolist(), *[x.tolist() for x in sc])
    assert is_u64(got, 16, 4)
    untouched(rec, AssertionError, "Not a power of two", api.vanishing_points, 1, 3, c, w, s, z, ks, *sc)
    reaches(rec, "plk_plonk_vanishing_points", api.vanishing_points, BAD, 2, c, w, s, z, ks, *sc)
    other_status(rec, "plk_plonk_vanishing_points", api.vanishing_points, 1, 2, c, w, s, z, ks, *sc)


def test_permutation_polynomial(rec):
    ks, beta, gamma = limbs(6, 4), limbs(4, seed=2), limbs(4, seed=3)
    for rows, stride in itertools.product((6, 9), (1, 8)):
        w, s = limbs(rows, 4, 4, seed=4), limbs(6, 4 * stride, 4, seed=5)
        got = call(rec, ("plk_plonk_permutation_z", 0, 2, H(w[:6]), H(s), stride, H(ks), H(beta), H(gamma), OUT(), NULL), api.permutation_polynomial, 0, 4,
                   w.tolist(), s.reshape(-1), ks.tolist(), beta.tolist(), gamma, sigma_stride=stride)
        assert is_u64(got, 4, 4)
    w, s = limbs(6, 4, 4), limbs(6, 32, 4)
    untouched(rec, AssertionError, "sigma_stride must be 1 or 8", api.permutation_polynomial, 0, 4, w, s, ks, beta, gamma, sigma_stride=2)
    untouched(rec, AssertionError, "Not a power of two", api.permutation_polynomial, 0, 3, w, s, ks, beta, gamma)
    refused(rec, api.permutation_polynomial, 0, 4, w[:5], s, ks, beta, gamma)
    panics(rec, "plk_plonk_permutation_z", "No inverse: row 2", AssertionError, "No inverse", api.permutation_polynomial, 0, 4, w, s, ks, beta, gamma)
    reaches(rec, "plk_plonk_permutation_z", api.permutation_polynomial, BAD, 4, w, s, ks, beta, gamma)
    other_status(rec, "plk_plonk_permutation_z", api.permutation_polynomial, 0, 4, w, s, ks, beta, gamma)


def test_wire_partitions_to_sigma(rec):
    ks = limbs(6, 4)
    m, o = np.arange(5, dtype=np.uint32), np.array([0, 2, 5], dtype=np.uint32)
    sigma, values = call(rec, ("plk_plonk_sigma", 1, 0, H(m, np.uint32), H(o, np.uint32), 2, H(ks), OUT(0), OUT(1)), api.wire_partitions_to_sigma, 0, 2, m.tolist(),
                         o.tolist(), ks.tolist())
    assert sigma.shape == (12,) and sigma.dtype == np.uint32 and is_u64(values, 6, 2, 4)
    sigma = call(rec, ("plk_plonk_sigma", 1, 0, H(m, np.uint32), H(o, np.uint32), 2, H(ks), OUT(), NULL), api.wire_partitions_to_sigma, 0, 2, m, o, ks, want_values=False)
    assert sigma.shape == (12,) and sigma.dtype == np.uint32
    untouched(rec, AssertionError, "offsets holds num_partitions + 1 entries", api.wire_partitions_to_sigma, 0, 2, m, [], ks)
    untouched(rec, AssertionError, "offsets[num_partitions] must be the number of members", api.wire_partitions_to_sigma, 0, 2, m, [0, 2, 4], ks)
    untouched(rec, AssertionError, "Not a power of two", api.wire_partitions_to_sigma, 0, 3, m, o, ks)
    reaches(rec, "plk_plonk_sigma", api.wire_partitions_to_sigma, BAD, 2, m, o, ks)
    other_status(rec, "plk_plonk_sigma", api.wire_partitions_to_sigma, 0, 2, m, o, ks)


@pytest.mark.parametrize("text", ["Non-routed wires should not be in a partition containing other wires", "no entry found for key: wire 3",
                                  "wire id out of range: 99"])
def test_sigma_panics(rec, text):
    m, o = np.arange(5, dtype=np.uint32), np.array([0, 2, 5], dtype=np.uint32)
    panics(rec, "plk_plonk_sigma", text, AssertionError, text, api.wire_partitions_to_sigma, 0, 2, m, o, limbs(6, 4))


def test_sigma_polynomials(rec):
    ks = limbs(6, 4)
    ident_m, ident_o = np.arange(12, dtype=np.uint32), np.arange(13, dtype=np.uint32)
    got = call(rec, ("plk_plonk_sigma", 1, 0, H(ident_m, np.uint32), H(ident_o, np.uint32), 12, H(ks), ANYPTR, ANYPTR), api.sigma_polynomials, 0,
               list(range(11, -1, -1)), 2, ks)
    assert is_u64(got, 6, 2, 4) and got.flags["C_CONTIGUOUS"]
    untouched(rec, AssertionError, "sigma maps [6n] to [6n]", api.sigma_polynomials, 0, list(range(11)), 2, ks)
    untouched(rec, AssertionError, "sigma maps [6n] to [6n]", api.sigma_polynomials, 0, list(range(1, 13)), 2, ks)


# ---- Plookup ----
def test_plookup_sorted_multiset_host(rec):
    t = _poly(5, 3, 9)
    got, s = names(rec, api.plookup_sorted_multiset, _poly(9, 5), t)
    assert got == [] and is_u64(s, 5, 4) and s[:, 0].tolist() == [5, 5, 3, 9, 9]
    untouched(rec, AssertionError, "called `Option::unwrap()` on a `None` value: an element of f is not in t", api.plookup_sorted_multiset, _poly(4), t)


def _padded(f):
    return np.concatenate([f, np.zeros((1, 4), dtype=np.uint64)])


def test_plookup_sorted_multiset_device(rec):
    t = limbs(4, 4)
    for f in (limbs(4, 4, seed=3), limbs(3, 4, seed=3)):  # n + 1 rows, or the n the reference passes: a zero row is added
        sent = f if f.shape[0] == 4 else _padded(f)
        got = call(rec, ("plk_plookup_sorted_multiset", 2, 1, H(sent), H(t), OUT(), REF(ctypes.c_uint)), api.plookup_sorted_multiset_device, 1, f.tolist(), t.reshape(-1))
        assert is_u64(got, 7, 4)
    untouched(rec, AssertionError, "f has n or n + 1 rows", api.plookup_sorted_multiset_device, 1, limbs(2, 4), t)
    untouched(rec, AssertionError, "Not a power of two", api.plookup_sorted_multiset_device, 1, limbs(3, 4), limbs(3, 4))
    rec.reply("plk_plookup_sorted_multiset", rc=INVALID, error="called `Option::unwrap()` on a `None` value", write={5: 3})
    assert raises(rec, AssertionError, "called `Option::unwrap()` on a `None` value: 3 elements of f are not in t", api.plookup_sorted_multiset_device, 1, t, t) == [
        "plk_plookup_sorted_multiset"]
    key_error(rec, api.plookup_sorted_multiset_device, BAD, t, t)
    other_status(rec, "plk_plookup_sorted_multiset", api.plookup_sorted_multiset_device, 1, t, t)


def test_plookup_grand_polynomial(rec):
    t, s, beta, gamma = limbs(4, 4), limbs(7, 4, seed=2), limbs(4, seed=3), limbs(4, seed=4)
    for f in (limbs(4, 4, seed=5), limbs(3, 4, seed=5)):
        sent = f if f.shape[0] == 4 else _padded(f)
        want = ("plk_plookup_grand_product", 2, 1, H(sent), H(t), H(s), H(beta), H(gamma), OUT(), REF(ctypes.c_int))
        assert is_u64(call(rec, want, api.plookup_grand_polynomial, 1, f.tolist(), t, s.reshape(-1), beta.tolist(), gamma), 4, 4)
        for closes in (0, 1):
            rec.reply("plk_plookup_grand_product", write={8: closes})
            out, c = call(rec, want[:8] + (OUT(0), want[9]), api.plookup_grand_polynomial, 1, f, t, s, beta, gamma, return_closes=True)
            assert is_u64(out, 4, 4) and c is bool(closes)
    untouched(rec, AssertionError, "f has n or n + 1 rows", api.plookup_grand_polynomial, 1, limbs(2, 4), t, s, beta, gamma)
    untouched(rec, AssertionError, "s has 2 n + 1 rows", api.plookup_grand_polynomial, 1, t, t, s[:6], beta, gamma)
    untouched(rec, AssertionError, "Not a power of two", api.plookup_grand_polynomial, 1, t[:3], t[:3], s, beta, gamma)
    panics(rec, "plk_plookup_grand_product", "No inverse", AssertionError, "No inverse", api.plookup_grand_polynomial, 1, t, t, s, beta, gamma)
    key_error(rec, api.plookup_grand_polynomial, BAD, t, t, s, beta, gamma)
    other_status(rec, "plk_plookup_grand_product", api.plookup_grand_polynomial, 1, t, t, s, beta, gamma)


def test_plookup_vanishing_values(rec):
    v, sc = limbs(5, 8, 4), [limbs(4, seed=s) for s in (2, 3, 4)]
    got = call(rec, ("plk_plookup_vanishing_points", 1, 0, H(v), H(sc[0]), H(sc[1]), H(sc[2]), OUT()), api.plookup_vanishing_values, 0, v.tolist(), sc[0].tolist(), sc[1],
               sc[2].reshape(1, 4))
    assert is_u64(got, 8, 4)
    refused(rec, api.plookup_vanishing_values, 0, limbs(4, 8, 4), *sc)
    refused(rec, api.plookup_vanishing_values, 0, limbs(5, 8, 4).reshape(5, 32), *sc)
    untouched(rec, AssertionError, "Not a power of two", api.plookup_vanishing_values, 0, limbs(5, 12, 4), *sc)
    reaches(rec, "plk_plookup_vanishing_points", api.plookup_vanishing_values, BAD, v, *sc)
    other_status(rec, "plk_plookup_vanishing_points", api.plookup_vanishing_values, 0, v, *sc)


# ---- the opening step ----
def test_powers(rec):
    x = limbs(4)
    assert is_u64(call(rec, ("plk_field_powers", 1, H(x), 5, OUT()), api.powers, 1, x.tolist(), 5), 5, 4)
    reaches(rec, "plk_field_powers", api.powers, BAD, x, 5)
    other_status(rec, "plk_field_powers", api.powers, 1, x, 5)


def test_eval_polys(rec):
    for n_points in (1, 8):
        pts, p0, p1 = limbs(n_points, 4), limbs(3, 4, seed=2), limbs(0, 4)
        got = call(rec, ("plk_plonk_eval_polys", 0, 2, HA([p0, None]), H([3, 0]), n_points, H(pts), OUT()), api.eval_polys, 0, [p0.tolist(), p1], pts.reshape(-1))
        assert is_u64(got, n_points, 2, 4)
        assert is_u64(call(rec, ("plk_plonk_eval_polys", 0, 0, HA([None]), H([]), n_points, H(pts), OUT()), api.eval_polys, 0, [], pts), n_points, 0, 4)
    reaches(rec, "plk_plonk_eval_polys", api.eval_polys, BAD, [p0], pts)
    other_status(rec, "plk_plonk_eval_polys", api.eval_polys, 0, [p0], pts)


def test_reduce_polynomials(rec):
    p0, p1, sc = limbs(3, 4, seed=2), limbs(0, 4), limbs(2, 4)
    got = call(rec, ("plk_poly_reduce", 0, 2, HA([p0, None]), H([3, 0]), H(sc), 4, OUT()), api.reduce_polynomials, 0, [p0.tolist(), p1], sc.tolist(), 4)
    assert is_u64(got, 4, 4)
    assert is_u64(call(rec, ("plk_poly_reduce", 0, 0, HA([None]), H([]), H([]), 4, OUT()), api.reduce_polynomials, 0, [], [], 4), 4, 4)
    untouched(rec, AssertionError, "one scalar per polynomial", api.reduce_polynomials, 0, [p0, p1], limbs(3, 4), 4)
    untouched(rec, AssertionError, "polynomial longer than the degree", api.reduce_polynomials, 0, [p0, p1], sc, 2)
    reaches(rec, "plk_poly_reduce", api.reduce_polynomials, BAD, [p0, p1], sc, 4)
    other_status(rec, "plk_poly_reduce", api.reduce_polynomials, 0, [p0, p1], sc, 4)


def test_scale_polynomials(rec):
    p0, p1, alpha = limbs(4, 4, seed=2), limbs(3, 4, seed=3), limbs(4, seed=4)
    got = call(rec, [("plk_field_powers", 0, H(alpha), 2, ANYPTR), ("plk_poly_reduce", 0, 2, HA([p0[:3], p1]), H([3, 3]), ANYPTR, 3, OUT())], api.scale_polynomials, 0,
               [p0.tolist(), p1], alpha.tolist(), 3)
    assert is_u64(got, 3, 4)
    untouched(rec, AssertionError, "the reference indexes every polynomial up to degree", api.scale_polynomials, 0, [p0, p1], alpha, 4)
    reaches(rec, "plk_field_powers", api.scale_polynomials, BAD, [p0, p1], alpha, 3)


def test_build_halo_b_and_halo_s(rec):
    for n_points in (1, 8):
        pts, v = limbs(n_points, 4), limbs(4, seed=5)
        assert is_u64(call(rec, ("plk_halo_build_b", 0, n_points, H(pts), H(v), 4, OUT()), api.build_halo_b, 0, pts.reshape(-1), v.tolist(), 4), 4, 4)
    for k in (1, 2):
        us = limbs(k, 4)
        assert is_u64(call(rec, ("plk_halo_s", 0, k, H(us), OUT()), api.halo_s, 0, us.tolist()), 1 << k, 4)
    panics(rec, "plk_halo_s", "No inverse", AssertionError, "No inverse", api.halo_s, 0, us)
    reaches(rec, "plk_halo_build_b", api.build_halo_b, BAD, pts, v, 4)
    reaches(rec, "plk_halo_s", api.halo_s, BAD, us)
    other_status(rec, "plk_halo_build_b", api.build_halo_b, 0, pts, v, 4)
    other_status(rec, "plk_halo_s", api.halo_s, 0, us)


# ---- batch inversion ----
def test_batch_multiplicative_inverse(rec):
    for field, L in FIELDS:
        x = limbs(3, L)
        assert is_u64(call(rec, ("plk_field_batch_inverse", field, H(x), OUT(), 3), api.batch_multiplicative_inverse, field, x.tolist()), 3, L)
        inv, none = call(rec, ("plk_field_batch_inverse_opt", field, H(x), OUT(0), OUT(1), 3), api.batch_multiplicative_inverse_opt, field, x.reshape(-1))
        assert is_u64(inv, 3, L) and none.shape == (3,) and none.dtype == U8 and not none.any()
    panics(rec, "plk_field_batch_inverse", "No inverse", AssertionError, "No inverse", api.batch_multiplicative_inverse, 0, limbs(3, 4))
    key_error(rec, api.batch_multiplicative_inverse, BAD, limbs(3, 4))
    key_error(rec, api.batch_multiplicative_inverse_opt, BAD, limbs(3, 4))
    other_status(rec, "plk_field_batch_inverse", api.batch_multiplicative_inverse, 0, limbs(3, 4))
    other_status(rec, "plk_field_batch_inverse_opt", api.batch_multiplicative_inverse_opt, 0, limbs(3, 4))


# ---- canonical byte encodings ----
def test_field_bytes(rec):
    for field, L in FIELDS:
        x = limbs(2, L)
        got = call(rec, ("plk_field_to_bytes", field, H(x), 2, OUT()), api.field_to_bytes, field, x.tolist())
        assert got.shape == (2, 8 * L) and got.dtype == U8
        b = (np.arange(2 * 8 * L) % 251).astype(U8)
        assert is_u64(call(rec, ("plk_field_from_bytes", field, H(b, U8), 2, OUT()), api.field_from_bytes, field, b.tolist()), 2, L)
    panics(rec, "plk_field_from_bytes", "Out of range", ValueError, "Out of range", api.field_from_bytes, 0, np.zeros(32, dtype=U8))
    hip_error(rec, "plk_field_from_bytes", api.field_from_bytes, 0, np.zeros(32, dtype=U8))
    key_error(rec, api.field_to_bytes, BAD, limbs(2, 4))
    key_error(rec, api.field_from_bytes, BAD, np.zeros(32, dtype=U8))
    other_status(rec, "plk_field_to_bytes", api.field_to_bytes, 0, limbs(2, 4))


def test_point_bytes(rec):
    for (curve, L), zero in itertools.product(CURVES, (None, flags(2))):
        p = limbs(2, 2, L)
        got = call(rec, ("plk_curve_point_to_bytes", curve, H(p), NULL if zero is None else H(zero, U8), 2, OUT()), api.point_to_bytes, curve, p.tolist(), zero)
        assert got.shape == (2, 1 + 8 * L) and got.dtype == U8
    for curve, L in CURVES:
        b = (np.arange(2 * (1 + 8 * L)) % 251).astype(U8)
        xy, z = call(rec, ("plk_curve_point_from_bytes", curve, H(b, U8), 2, OUT(0), OUT(1), ANYPTR), api.point_from_bytes, curve, b.tolist())
        assert is_u64(xy, 2, 2, L) and z.shape == (2,) and z.dtype == U8 and not z.any()
        for rc in (0, INVALID):  # with_status: a refusal is an answer, the per-record status
            rec.reply("plk_curve_point_from_bytes", rc=rc, error="x is not on the curve")
            xy, z, st = call(rec, ("plk_curve_point_from_bytes", curve, H(b, U8), 2, OUT(0), OUT(1), OUT(2)), api.point_from_bytes, curve, b, with_status=True)
            assert is_u64(xy, 2, 2, L) and z.shape == (2,) and z.dtype == U8 and st.shape == (2,) and st.dtype == U8 and not st.any()
    b = np.zeros(33, dtype=U8)
    panics(rec, "plk_curve_point_from_bytes", "x is not on the curve", ValueError, "x is not on the curve", api.point_from_bytes, 0, b)
    hip_error(rec, "plk_curve_point_from_bytes", api.point_from_bytes, 0, b)
    hip_error(rec, "plk_curve_point_from_bytes", api.point_from_bytes, 0, b, with_status=True)
    key_error(rec, api.point_to_bytes, BAD, limbs(2, 2, 4))
    key_error(rec, api.point_from_bytes, BAD, b)
    other_status(rec, "plk_curve_point_to_bytes", api.point_to_bytes, 0, limbs(2, 2, 4))


# ---- the BLAKE3 hash to the curve ----
def test_blake_field(rec):
    for field, L in FIELDS:
        seeds = limbs(3, L)
        for iters, sent in ((2, [2, 2, 2]), ([1, 2, 3], [1, 2, 3]), (np.array([7], dtype=np.int64), [7, 7, 7])):  # one for all, or one per row
            x, y_neg = call(rec, ("plk_blake_field", 3, field, H(sent, U8), H(seeds), OUT(0), OUT(1)), api.blake_field, field, iters, seeds.tolist())
            assert is_u64(x, 3, L) and y_neg.shape == (3,) and y_neg.dtype == U8 and not y_neg.any()
    panics(rec, "plk_blake_field", "no point after 256 tries", ValueError, "no point after 256 tries", api.blake_field, 0, 0, limbs(3, 4))
    hip_error(rec, "plk_blake_field", api.blake_field, 0, 0, limbs(3, 4))
    key_error(rec, api.blake_field, BAD, 0, limbs(3, 4))


def test_blake_hash_to_curve(rec):
    for curve, L in CURVES:
        seeds = limbs(3, L)
        assert is_u64(call(rec, ("plk_hash_field_to_curve", 3, curve, H(seeds), OUT()), api.blake_hash_base_field_to_curve, curve, seeds.tolist()), 3, 2, L)
        assert is_u64(call(rec, ("plk_hash_to_curve", 1, curve, 9, OUT()), api.blake_hash_usize_to_curve, curve, 9), 2, L)  # count=None: the point itself
        assert is_u64(call(rec, ("plk_hash_to_curve", 1, curve, 9, OUT()), api.blake_hash_usize_to_curve, curve, 9, 1), 1, 2, L)
        assert is_u64(call(rec, ("plk_hash_to_curve", 3, curve, 9, OUT()), api.blake_hash_usize_to_curve, curve, np.int64(9), count=3), 3, 2, L)
        rec.calls, rec.want = [], [("plk_hash_to_curve", 6, curve, 0, ANYPTR)]
        g, h, u = api.pedersen_generators(curve, 4)
        assert rec.calls == [("plk_hash_to_curve", 6, curve, 0, ANYPTR)] and is_u64(g, 4, 2, L) and is_u64(h, 2, L) and is_u64(u, 2, L)
    panics(rec, "plk_hash_field_to_curve", "no point", ValueError, "no point", api.blake_hash_base_field_to_curve, 0, limbs(3, 4))
    panics(rec, "plk_hash_to_curve", "no point", ValueError, "no point", api.blake_hash_usize_to_curve, 0, 9)
    hip_error(rec, "plk_hash_field_to_curve", api.blake_hash_base_field_to_curve, 0, limbs(3, 4))
    hip_error(rec, "plk_hash_to_curve", api.blake_hash_usize_to_curve, 0, 9)
    key_error(rec, api.blake_hash_base_field_to_curve, BAD, limbs(3, 4))
    key_error(rec, api.blake_hash_usize_to_curve, BAD, 9)
    key_error(rec, api.pedersen_generators, BAD, 4)


# ---- Rescue ----
def test_rescue_rounds_and_mds(rec):
    rec.reply("plk_rescue_rounds", write={2: 16})
    got = call(rec, ("plk_rescue_rounds", 4, 128, REF(ctypes.c_size_t)), api.rescue_rounds, 4.0, np.int64(128))
    assert got == 16 and type(got) is int
    panics(rec, "plk_rescue_rounds", "width 0", ValueError, "width 0", api.rescue_rounds, 0, 128)
    hip_error(rec, "plk_rescue_rounds", api.rescue_rounds, 4, 128)
    for field, L in FIELDS:
        assert is_u64(call(rec, ("plk_rescue_mds", 4, field, OUT()), api.rescue_mds, field), 4, 4, L)
        assert is_u64(call(rec, ("plk_rescue_mds", 3, field, OUT()), api.rescue_mds, field, width=3), 3, 3, L)
    panics(rec, "plk_rescue_mds", "unknown field 9", ValueError, "unknown field 9", api.rescue_mds, BAD)  # the bad id goes to the library, as 4 limbs
    assert is_u64(call(rec, ("plk_rescue_mds", 4, BAD, OUT()), api.rescue_mds, BAD), 4, 4, 4)
    hip_error(rec, "plk_rescue_mds", api.rescue_mds, 0)


def test_rescue_context(rec):
    for field, L in FIELDS:
        c = limbs(3, 2, 4, L)
        rec.reply("plk_rescue_create", write={4: 0xABCD})
        ctx = call(rec, ("plk_rescue_create", 4, field, 3, H(c), REF(ctypes.c_void_p)), api.RescueContext, field, c.tolist())
        assert (ctx.field, ctx.width, ctx.rounds) == (field, 4, 3) and isinstance(ctx.handle, ctypes.c_void_p) and ctx.handle.value == 0xABCD
        rec.reply("plk_rescue_free", rc=HIP, error="hipErrorUnknown")  # plk_rescue_free's status is checked, and the handle is kept
        assert raises(rec, lib.PlonkyHipError, "libplonky_hip error %d: hipErrorUnknown" % HIP, ctx.free) == ["plk_rescue_free"]
        call(rec, ("plk_rescue_free", HND(0xABCD)), ctx.free)
        assert ctx._ctx is None and names(rec, ctx.free)[0] == []
        untouched(rec, AssertionError, "the context has been freed", lambda: ctx.handle)
        rec.reply("plk_rescue_create", write={4: 0xABCD})
        with call(rec, ("plk_rescue_create", 3, field, 2, H(c[:2, :, :3]), REF(ctypes.c_void_p)), api.RescueContext, field, c[:2, :, :3], width=3, rounds=2) as ctx:
            assert (ctx.width, ctx.rounds) == (3, 2)
        assert [c_[0] for c_ in rec.calls] == ["plk_rescue_free"] and ctx._ctx is None  # freed on the way out of the with block
        rec.calls = []
        ctx = api.RescueContext(field, c)  # the recorder hands out no handle: nothing to free
        rec.calls = []
        assert names(rec, ctx.free)[0] == []
    untouched(rec, AssertionError, "constants: rounds x 2 x width elements", api.RescueContext, 0, limbs(3, 2, 4, 4), rounds=2)
    panics(rec, "plk_rescue_create", "unknown field 9", ValueError, "unknown field 9", api.RescueContext, BAD, limbs(3, 2, 4, 4))  # reaches the library, as 4 limbs
    hip_error(rec, "plk_rescue_create", api.RescueContext, 0, limbs(3, 2, 4, 4))


def _ctx(field, width=4):
    return SimpleNamespace(field=field, width=width, handle=HANDLE)


def test_rescue_permutation_and_sponge(rec):
    for field, L in FIELDS:
        states = limbs(2, 4, L)
        assert is_u64(call(rec, ("plk_rescue_permutation", 2, HANDLE, H(states), OUT()), api.rescue_permutation, _ctx(field), states.tolist()), 2, 4, L)
        assert is_u64(call(rec, ("plk_rescue_permutation", 1, HANDLE, H(states[0]), OUT()), api.rescue_permutation, _ctx(field), states[0]), 4, L)  # one state
        inputs = limbs(2, 3, L)
        assert is_u64(call(rec, ("plk_rescue_sponge", 2, HANDLE, 3, H(inputs), 2, OUT()), api.rescue_sponge, _ctx(field), inputs.tolist(), np.int64(2)), 2, 2, L)
        assert is_u64(call(rec, ("plk_rescue_sponge", 1, HANDLE, 3, H(inputs[0]), 2, OUT()), api.rescue_sponge, _ctx(field), inputs[0], 2), 2, L)  # one row
        assert is_u64(call(rec, ("plk_rescue_sponge", 2, HANDLE, 0, H([]), 2, OUT()), api.rescue_sponge, _ctx(field), limbs(2, 0, L), 2), 2, 2, L)
        for k, fn in ((1, api.rescue_hash_n_to_1), (2, api.rescue_hash_n_to_2), (3, api.rescue_hash_n_to_3)):
            assert is_u64(call(rec, ("plk_rescue_sponge", 2, HANDLE, 3, H(inputs), k, OUT()), fn, _ctx(field), inputs), 2, k, L)
    refused(rec, api.rescue_permutation, _ctx(0), limbs(2, 3, 4))
    refused(rec, api.rescue_permutation, _ctx(0), limbs(2, 4, 6))
    refused(rec, api.rescue_sponge, _ctx(0), limbs(2, 3, 6), 2)
    refused(rec, api.rescue_sponge, _ctx(0), limbs(12), 2)
    panics(rec, "plk_rescue_permutation", "bad context", ValueError, "bad context", api.rescue_permutation, _ctx(0), limbs(2, 4, 4))
    panics(rec, "plk_rescue_sponge", "bad context", ValueError, "bad context", api.rescue_sponge, _ctx(0), limbs(2, 3, 4), 2)
    hip_error(rec, "plk_rescue_permutation", api.rescue_permutation, _ctx(0), limbs(2, 4, 4))
    hip_error(rec, "plk_rescue_sponge", api.rescue_sponge, _ctx(0), limbs(2, 3, 4), 2)
    key_error(rec, api.rescue_permutation, _ctx(BAD), limbs(2, 4, 4))
    key_error(rec, api.rescue_sponge, _ctx(BAD), limbs(2, 3, 4), 2)


def test_rescue_hash_to_curve(rec):
    ctx = SimpleNamespace(handle=HANDLE)
    for curve, L in CURVES:
        seeds = limbs(3, L)
        assert is_u64(call(rec, ("plk_rescue_hash_field_to_curve", 3, HANDLE, curve, H(seeds), OUT()), api.hash_base_field_to_curve, ctx, curve, seeds.tolist()), 3, 2, L)
        assert is_u64(call(rec, ("plk_rescue_hash_field_to_curve", 1, HANDLE, curve, H(seeds[0]), OUT()), api.hash_base_field_to_curve, ctx, curve, seeds[0]), 2, L)
        for fn in (api.hash_usize_to_curve, api.hash_u32_to_curve):
            assert is_u64(call(rec, ("plk_rescue_hash_to_curve", 1, HANDLE, curve, 9, OUT()), fn, ctx, curve, 9), 2, L)  # count=None: the point itself
            assert is_u64(call(rec, ("plk_rescue_hash_to_curve", 1, HANDLE, curve, 9, OUT()), fn, ctx, curve, 9, 1), 1, 2, L)
            assert is_u64(call(rec, ("plk_rescue_hash_to_curve", 3, HANDLE, curve, 9, OUT()), fn, ctx, curve, np.int64(9), count=3), 3, 2, L)
    untouched(rec, ValueError, "seeds -1 .. -1 do not fit a u32", api.hash_u32_to_curve, ctx, 0, -1)
    untouched(rec, ValueError, "seeds 4294967295 .. 4294967296 do not fit a u32", api.hash_u32_to_curve, ctx, 0, (1 << 32) - 1, 2)
    panics(rec, "plk_rescue_hash_field_to_curve", "no point", ValueError, "no point", api.hash_base_field_to_curve, ctx, 0, limbs(3, 4))
    panics(rec, "plk_rescue_hash_to_curve", "no point", ValueError, "no point", api.hash_usize_to_curve, ctx, 0, 9)
    hip_error(rec, "plk_rescue_hash_field_to_curve", api.hash_base_field_to_curve, ctx, 0, limbs(3, 4))
    hip_error(rec, "plk_rescue_hash_to_curve", api.hash_usize_to_curve, ctx, 0, 9)
    key_error(rec, api.hash_base_field_to_curve, ctx, BAD, limbs(3, 4))
    assert is_u64(call(rec, ("plk_rescue_hash_to_curve", 2, HANDLE, BAD, 9, OUT()), api.hash_usize_to_curve, ctx, BAD, 9, 2), 2, 2, 4)  # reaches the library, as 4 limbs
    assert is_u64(call(rec, ("plk_rescue_hash_to_curve", 2, HANDLE, BAD, 9, OUT()), api.hash_u32_to_curve, ctx, BAD, 9, 2), 2, 2, 4)


def test_kth_root(rec):
    for field, L in FIELDS:
        x = limbs(3, L)
        got = call(rec, ("plk_field_kth_root", 3, field, 5, P(x), OUT()), api.kth_root, field, x, 5.0)
        assert is_u64(got, 3, L)
    assert is_u64(call(rec, ("plk_field_kth_root", 1, 0, 5, H(x[0, :4]), OUT()), api.kth_root, 0, x[0, :4].tolist(), 5), 4)  # the shape of x comes back
    panics(rec, "plk_field_kth_root", "k divides p - 1", ValueError, "k divides p - 1", api.kth_root, 0, limbs(3, 4), 3)
    hip_error(rec, "plk_field_kth_root", api.kth_root, 0, limbs(3, 4), 5)
    assert is_u64(call(rec, ("plk_field_kth_root", 3, BAD, 5, ANYPTR, OUT()), api.kth_root, BAD, limbs(3, 4), 5), 3, 4)  # reaches the library, as 4 limbs


def test_challenger(rec):
    for field, L in FIELDS:
        ch = api.Challenger(_ctx(field))
        assert is_u64(ch.sponge_state, 4, L) and not ch.sponge_state.any()
        ch.observe_elements(limbs(2, L))
        ch.observe_affine_point(limbs(2, L, seed=3))  # four elements: a chunk of three and a chunk of one
        assert rec.calls == [] and len(ch.input_buffer) == 4
        got, c = names(rec, ch.get_challenge)
        assert got == ["plk_field_op", "plk_rescue_permutation"] * 2 and is_u64(c, L) and len(ch.output_buffer) == 2 and ch.input_buffer == []
        got, (c1, c2) = names(rec, ch.get_2_challenges)  # nothing observed: no call, the buffer is refilled from the state
        assert got == [] and is_u64(c1, L) and is_u64(c2, L)
        d = ch.clone()
        d.observe_element(limbs(L))
        assert d.output_buffer == [] and len(ch.output_buffer) == 2 and d.ctx is ch.ctx
        assert names(rec, d.get_n_challenges, 3)[0] == ["plk_field_op", "plk_rescue_permutation"]
        untouched(rec, ValueError, None, ch.observe_element, limbs(L + 1))  # numpy's own: cannot reshape
    untouched(rec, KeyError, None, api.Challenger, _ctx(BAD))


def test_challenger_call_content(rec):
    ch = api.Challenger(_ctx(0))
    e = limbs(2, 4)
    ch.observe_elements(e.tolist())
    zeros = np.zeros((2, 4), dtype=np.uint64)
    rec.calls, rec.want = [], [("plk_field_op", 0, 0, H(zeros), H(e), ANYPTR, 2), ("plk_rescue_permutation", 1, HANDLE, ANYPTR, ANYPTR)]
    ch.get_challenge()
    assert rec.calls == rec.want


# ---- a point times a scalar of its own, the Halo endomorphism ----
def test_curve_scalar_mul_and_halo_n_mul(rec):
    for (curve, L), (ns, npts), with_flags in itertools.product(CURVES, ((1, 1), (3, 3), (1, 3), (3, 1)), (False, True)):
        count = max(ns, npts)
        s, p = limbs(ns, 4), limbs(npts, 2, L, seed=3)
        zero = flags(npts) if with_flags else None
        zp = H(zero, U8) if with_flags else NULL
        out, oz = call(rec, ("plk_curve_scalar_mul", count, curve, ns, H(s), npts, H(p), zp, OUT(0), OUT(1)), api.curve_scalar_mul, curve, s.tolist(), p.reshape(-1),
                       None if zero is None else zero.reshape(-1, 1))
        assert is_u64(out, count, 2, L) and not out.any() and oz.shape == (count,) and oz.dtype == U8 and not oz.any()
        out, oz = call(rec, ("plk_halo_n_mul", count, curve, 100, ns, H(s), npts, H(p), zp, OUT(0), OUT(1)), api.halo_n_mul, curve, s, p.tolist(), zero=zero,
                       security_bits=100.0)
        assert is_u64(out, count, 2, L) and oz.shape == (count,) and oz.dtype == U8
    out, oz = call(rec, ("plk_halo_n_mul", 1, 0, 128, 1, ANYPTR, 1, ANYPTR, NULL, OUT(0), OUT(1)), api.halo_n_mul, 0, limbs(4), limbs(2, 4))
    for fn, entry in ((api.curve_scalar_mul, "plk_curve_scalar_mul"), (api.halo_n_mul, "plk_halo_n_mul")):
        refused(rec, fn, 0, limbs(2, 4), limbs(2, 2, 4), flags(3))
        panics(rec, entry, "1 or count scalars", ValueError, "1 or count scalars", fn, 0, limbs(2, 4), limbs(3, 2, 4))
        hip_error(rec, entry, fn, 0, limbs(2, 4), limbs(2, 2, 4))
        key_error(rec, fn, BAD, limbs(2, 4), limbs(2, 2, 4))


def test_halo_n(rec):
    s = limbs(3, 4)
    assert is_u64(call(rec, ("plk_halo_n", 3, 2, 128, H(s), OUT()), api.halo_n, 2, s.tolist()), 3, 4)
    assert is_u64(call(rec, ("plk_halo_n", 1, 0, 64, H(s[0]), OUT()), api.halo_n, 0, s[0], security_bits=64.0), 1, 4)
    panics(rec, "plk_halo_n", "security_bits", ValueError, "security_bits", api.halo_n, 0, s, 300)
    hip_error(rec, "plk_halo_n", api.halo_n, 0, s)
    reaches(rec, "plk_halo_n", api.halo_n, BAD, s)


def test_halo_g(rec):
    x, us = limbs(4), limbs(2, 4, seed=3)
    got, g = names(rec, api.halo_g, 1, x.tolist(), us.reshape(-1))
    assert got == ["plk_field_powers"] + ["plk_field_op"] * 10 and is_u64(g, 4)
    rec.calls, rec.want = [], [("plk_field_powers", 1, H(x), 1, ANYPTR), ("plk_field_op", 1, 2, H(us[1]), H(x), ANYPTR, 1), ("plk_field_op", 1, 5, H(us[1]), H(us[1]), ANYPTR, 1)]
    api.halo_g(1, x, us)
    assert rec.calls[:3] == rec.want and [c[2] for c in rec.calls[1:]] == [2, 5, 0, 2, 4] * 2  # mul, inverse, add, mul, square per challenge, last first
    reaches(rec, "plk_field_powers", api.halo_g, BAD, x, us[:0])


# ---- the group side of the verifier: sequences of calls ----
def _pt(L, seed):
    return limbs(2, L, seed=seed)


def test_schnorr_protocol(rec):
    for curve, L in CURVES:
        rec.reply("plk_curve_scalar_field", rc=1)
        sc = [limbs(4, seed=s) for s in range(6)]
        got, (r, z1, z2) = names(rec, api.schnorr_protocol, curve, sc[0], sc[1], _pt(L, 7), sc[2], (_pt(L, 8), 0), _pt(L, 9).tolist(), sc[3], sc[4].tolist(), sc[5])
        assert got == ["plk_curve_scalar_field", "plk_curve_scalar_mul", "plk_curve_sum_affine", "plk_curve_scalar_mul", "plk_curve_sum_affine"] + ["plk_field_op"] * 4
        assert is_u64(r[0], 2, L) and r[1] == 0 and is_u64(z1, 4) and is_u64(z2, 4)
    # the first calls, literally: the scalar field the library names is the one the z's are computed in
    rec.reply("plk_curve_scalar_field", rc=1)
    rec.calls, rec.want = [], [("plk_curve_scalar_field", 0), ("plk_curve_scalar_mul", 1, 0, 1, H(sc[1]), 1, H(_pt(4, 8)), H([1], U8), ANYPTR, ANYPTR)]
    api.schnorr_protocol(0, sc[0], sc[1], _pt(4, 7), sc[2], (_pt(4, 8), 1), _pt(4, 9), sc[3], sc[4], sc[5])
    assert rec.calls[:2] == rec.want and [c[1] for c in rec.calls[5:]] == [1, 1, 1, 1] and [c[2] for c in rec.calls[5:]] == [2, 0, 2, 0]
    assert raises(rec, KeyError, None, api.schnorr_protocol, BAD, sc[0], sc[1], _pt(4, 7), sc[2], _pt(4, 8), _pt(4, 9), sc[3], sc[4], sc[5]) == ["plk_curve_scalar_field"]


def test_verify_ipa(rec):
    sequence = (["plk_curve_scalar_field", "plk_curve_scalar_mul", "plk_curve_sum_affine"] + ["plk_field_op"] * 3
                + ["plk_msm_precompute_ex", "plk_msm_execute", "plk_msm_free"] + ["plk_curve_sum_affine"] * 2 + ["plk_curve_scalar_mul"] + ["plk_curve_sum_affine"] * 2)
    for curve, L in CURVES:
        sc = [limbs(4, seed=s) for s in range(6)]
        us, ls, rs = limbs(2, 4, seed=11), limbs(2, 2, L, seed=12), limbs(2, 2, L, seed=13)
        args = lambda l, r: (curve, l, r, _pt(L, 7), (_pt(L, 8), 0), sc[0], sc[1], us, _pt(L, 9), _pt(L, 10), sc[2], ((_pt(L, 14), 0), sc[3], sc[4]))
        for l, r in ((ls, rs), ((ls, flags(2)), (rs.tolist(), [0, 0]))):
            rec.reply("plk_curve_scalar_field", rc=1)
            rec.reply("plk_msm_precompute_ex", write={6: 0xBEEF})
            got, ok = names(rec, api.verify_ipa, *args(l, r))
            assert got == sequence and type(ok) is bool
    assert raises(rec, AssertionError, "one L_j and one R_j per challenge", api.verify_ipa, *args(ls[:1], rs)) == ["plk_curve_scalar_field"]


def test_verify_halo_g(rec):
    for curve, L in CURVES:
        us = limbs(2, 4)
        rec.reply("plk_curve_scalar_field", rc=1)
        ok = call(rec, [("plk_curve_scalar_field", curve), ("plk_halo_s", 1, 2, H(us), ANYPTR), ("plk_msm_execute", CTX, ANYPTR, 4, ANYPTR, ANYPTR)], api.verify_halo_g,
                  curve, (_pt(L, 3), 0), us, _pre(curve, 4))
        assert type(ok) is bool
    rec.reply("plk_curve_scalar_field", rc=1)
    assert raises(rec, AssertionError, "2^len(halo_us) generators", api.verify_halo_g, 0, _pt(4, 3), us, _pre(0, 8)) == ["plk_curve_scalar_field", "plk_halo_s"]


# ---- the layer itself: the names other modules import ----
def test_names_that_other_modules_import():
    assert api._FIELD_LIMBS == {0: 4, 1: 4, 2: 4, 3: 6, 4: 4, 5: 4} and api._CURVE_LIMBS == {0: 4, 1: 4, 2: 6, 3: 4, 4: 4}
    assert api.CURVE_SCALAR_FIELD == {0: 1, 1: 0, 2: 2, 3: 5, 4: 4} and api.CURVE_BASE_FIELD == {0: 0, 1: 1, 2: 3, 3: 4, 4: 5}
    x = limbs(2, 4)
    assert api._u64(x) is x and api._u64(x.tolist(), 8).shape == (8,) and api._u64(x.tolist()).dtype == np.uint64
    p = api._ptr(x)
    assert isinstance(p, ctypes.c_void_p) and p.value == x.ctypes.data
    assert [api.log2_strict(1 << k) for k in range(4)] == [0, 1, 2, 3] and api.log2_ceil(5) == 3
    with pytest.raises(AssertionError, match="Not a power of two"):
        api.log2_strict(12)
