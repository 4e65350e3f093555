"""CPU-only: what plonky_amd.device hands to the C ABI, pinned from outside.  The library is replaced by a recorder, _stream by a
constant and the tensors by CPU tensors that report is_cuda; every test states the C call it expects literally - the entry point, the
arguments and their order - and the refusals check that nothing reaches the library.  libplonky_hip.so is never loaded.

Device pointers are compared with data_ptr(), host limbs by their content read back through the pointer while the wrapper's array
is alive, scalars and sizes by value.  A null pointer counts as one however it is spelt (None or a c_void_p of None)."""
import ctypes
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from plonky_amd import device
from tests.abi_recorder import ANYPTR, H, NULL, OUT, P, PA, REF, _Recorder, call, refused

STREAM, CTX, TABLES, HANDLE = "stream", "ctx", "tables-ctx", "rescue-handle"
NO = ctypes.c_size_t(-1).value
FIELDS = ((0, 4), (3, 6))  # (field id, limbs): TweedledeeBase, Bls12377Base
CURVES = ((0, 4), (2, 6))  # (curve id, limbs): Tweedledee, Bls12377


class _Dev(torch.Tensor):
    is_cuda = True


def dev(*shape, dtype=torch.int64):
    return torch.zeros(shape, dtype=dtype).as_subclass(_Dev)


def cpu(*shape, dtype=torch.int64):
    return torch.zeros(shape, dtype=dtype)


def strided(*shape, dtype=torch.int64):
    """the same shape, on the 'device', not contiguous"""
    t = dev(*shape[:-1], 2 * shape[-1], dtype=dtype)[..., ::2]
    assert tuple(t.shape) == shape and not t.is_contiguous()
    return t


def limbs(*shape, seed=1):
    return (np.arange(int(np.prod(shape)), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)).reshape(shape)


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(device._lib, "load", lambda: r)
    monkeypatch.setattr(device, "_stream", lambda: STREAM)
    return r


def bad_tensors(*shape, dtype=torch.int64, wrong_dtype=torch.int32):
    """one fault at a time: on the CPU, not contiguous, of another dtype"""
    return [cpu(*shape, dtype=dtype), strided(*shape, dtype=dtype), dev(*shape, dtype=wrong_dtype)]


# ---- transforms and polynomial products ----
def test_ntt_dev(rec):
    for (field, L), log_n, lead, inverse in itertools.product(FIELDS, (1, 2), ((), (1,), (2,)), (False, True)):
        n = 1 << log_n
        x, out = dev(*lead, n, L), dev(*lead, n, L)
        got = call(rec, ("plk_ntt_dev", field, log_n, 1 if inverse else 0, lead[0] if lead else 1, P(x), P(out), STREAM),
                   device.ntt_dev, field, x, inverse=inverse, out=out)
        assert got is out
    for x in bad_tensors(2, 4) + [dev(2, 5)]:
        refused(rec, device.ntt_dev, 0, x, out=dev(2, 4))
    refused(rec, device.ntt_dev, 0, dev(3, 4), out=dev(3, 4))  # Not a power of two


def test_ntt_padded_dev(rec):
    for (field, L), (lead, length, log_n) in itertools.product(FIELDS, (((), 2, 1), ((1,), 3, 2), ((2,), 0, 2), ((2, 3), 1, 1))):
        x, out = dev(*lead, length, L), dev(*lead, 1 << log_n, L)
        got = call(rec, ("plk_ntt_padded_dev", field, log_n, int(np.prod(lead, dtype=np.int64)), P(x), length, length, P(out), STREAM),
                   device.ntt_padded_dev, field, x, log_n, out=out)
        assert got is out
    for x in bad_tensors(2, 4) + [dev(2, 6)]:
        refused(rec, device.ntt_padded_dev, 0, x, 1, out=dev(2, 4))


def test_divide_by_z_h_dev(rec):
    for length, rows in ((1, 1), (5, 8), (5, 9), (8, 8)):
        coeffs, out = dev(length, 4), dev(rows, 4)
        got = call(rec, ("plk_poly_divide_by_z_h_dev", 1, P(coeffs), length, 2, P(out), rows, REF(ctypes.c_size_t), STREAM),
                   device.divide_by_z_h_dev, 1, coeffs, 2, out=out)
        assert got.shape == (0, 4)  # the recorder leaves out_len at 0
    for x in bad_tensors(5, 4) + [dev(5, 6)]:
        refused(rec, device.divide_by_z_h_dev, 1, x, 2, out=dev(8, 4))
    refused(rec, device.divide_by_z_h_dev, 1, dev(5, 4), 2, out=dev(7, 4))


def test_poly_mul_dev(rec):
    a, b = dev(3, 4), dev(2, 4)
    call(rec, ("plk_poly_mul_dev", 0, P(a), 3, P(b), 2, ANYPTR, 8, REF(ctypes.c_size_t), STREAM), device.poly_mul_dev, 0, a, b)
    for x in bad_tensors(2, 4) + [dev(2, 6)]:
        refused(rec, device.poly_mul_dev, 0, a, x)
        refused(rec, device.poly_mul_dev, 0, x, a)


# ---- generators and the MSM ----
def test_gen_bases_dev(rec):
    for curve, L in CURVES:
        g0, d = limbs(2, L), limbs(2, L, seed=7)
        got = call(rec, ("plk_curve_gen_bases_dev", curve, 3, 5, H(g0), H(d), OUT(), STREAM), device.gen_bases_dev, curve, 3, g0, d, first=5,
                   device="cpu")
        assert got.shape == (3, 2, L) and got.dtype == torch.int64


def test_hash_to_curve_dev(rec):
    for (curve, L), count in itertools.product(CURVES, (1, 2)):
        out, seeds = dev(count, 2, L), dev(count, L)
        assert call(rec, ("plk_hash_to_curve_dev", count, curve, 9, P(out), STREAM), device.hash_to_curve_dev, curve, count, seed_start=9, out=out) is out
        assert call(rec, ("plk_hash_field_to_curve_dev", count, curve, P(seeds), P(out), STREAM), device.hash_to_curve_dev, curve, count, seeds=seeds,
                    out=out) is out
    for s in bad_tensors(2, 4) + [dev(3, 4), dev(2, 6), dev(8)]:
        refused(rec, device.hash_to_curve_dev, 0, 2, seeds=s, out=dev(2, 2, 4))
    for o in bad_tensors(2, 2, 4) + [dev(3, 2, 4), dev(2, 2, 6), dev(16)]:
        refused(rec, device.hash_to_curve_dev, 0, 2, out=o)
        refused(rec, device.hash_to_curve_dev, 0, 2, seeds=dev(2, 4), out=o)
    refused(rec, device.hash_to_curve_dev, 0, 2, device="cpu")  # a fresh out that is not on a GPU


def test_msm_precompute_dev(rec):
    for (curve, L), n in itertools.product(CURVES, (1, 8)):
        bases, zero = dev(n, 2, L), dev(n, dtype=torch.uint8)
        pre = call(rec, ("plk_msm_precompute_dev_ex", curve, n, P(bases), NULL, 0, 0, STREAM, REF(ctypes.c_void_p)), device.msm_precompute_dev, curve, bases)
        assert (pre.curve, pre.n, pre.w) == (curve, n, 11) and isinstance(pre._ctx, ctypes.c_void_p)
        pre = call(rec, ("plk_msm_precompute_dev_ex", curve, n, P(bases), P(zero), 13, 1, STREAM, REF(ctypes.c_void_p)),
                   device.msm_precompute_dev, curve, bases, w=8, zero=zero, device_window=13, table_free=True)
        assert (pre.n, pre.w) == (n, 8)
    for b in bad_tensors(2, 2, 4):
        refused(rec, device.msm_precompute_dev, 0, b)


def test_msm_execute_dev(rec):
    for (curve, L), (lead, n), projective in itertools.product(CURVES, (((), 1), ((1,), 8), ((2,), 8), ((), 0)), (False, True)):
        pre = SimpleNamespace(_ctx=CTX, n=n, curve=curve)
        batch = lead[0] if lead else 1
        scalars, xy, z = dev(*lead, n, 4), dev(batch, 3 if projective else 2, L), dev(batch, dtype=torch.uint8)
        entry = "plk_msm_execute_projective_dev" if projective else "plk_msm_execute_dev"
        got = call(rec, (entry, CTX, batch, P(scalars), n, P(xy), P(z), STREAM), device.msm_execute_dev, pre, scalars, out_xy=xy, out_zero=z,
                   projective=projective)
        assert got[0] is xy and got[1] is z
    pre = SimpleNamespace(_ctx=CTX, n=8, curve=0)
    for s in bad_tensors(8, 4):
        refused(rec, device.msm_execute_dev, pre, s, out_xy=dev(1, 2, 4), out_zero=dev(1, dtype=torch.uint8))
    with pytest.raises(AssertionError, match=r"powers_per_generator\.len\(\) != scalars\.len\(\)"):
        device.msm_execute_dev(pre, dev(7, 4), out_xy=dev(1, 2, 4), out_zero=dev(1, dtype=torch.uint8))
    assert rec.calls == []
    refused(rec, device.msm_execute_dev, pre, dev(8, 4), out_xy=dev(1, 2, 4), out_zero=dev(1, dtype=torch.uint8), projective=True)


def test_msm_execute_parts_dev(rec):
    for curve, L in CURVES:
        pre = SimpleNamespace(_ctx=CTX, n=8, curve=curve)
        for parts in ([(0, dev(8, 4))], [(0, dev(3, 4)), (5, dev(2, 4))]):
            batch = len(parts)
            xy, z = dev(batch, 2, L), dev(batch, dtype=torch.uint8)
            first, count, ptrs = H([p[0] for p in parts]), H([p[1].shape[0] for p in parts]), PA([p[1] for p in parts])
            got = call(rec, ("plk_msm_execute_parts_dev", CTX, batch, first, count, ptrs, P(xy), P(z), STREAM), device.msm_execute_parts_dev, pre, parts,
                       out_xy=xy, out_zero=z)
            assert got[0] is xy and got[1] is z
            buckets = [(0, 1), (1, 2)][:batch]
            bp, bn = H([b[0] for b in buckets], np.uint32), H([b[1] for b in buckets], np.uint32)
            got = call(rec, ("plk_msm_execute_parts_buckets_dev", CTX, batch, first, count, ptrs, bp, bn, P(xy), P(z), STREAM),
                       device.msm_execute_parts_dev, pre, parts, out_xy=xy, out_zero=z, buckets=buckets)
            assert got[0] is xy and got[1] is z
    pre = SimpleNamespace(_ctx=CTX, n=8, curve=0)
    outs = dict(out_xy=dev(2, 2, 4), out_zero=dev(2, dtype=torch.uint8))
    for t in bad_tensors(2, 4) + [dev(2, 3)]:
        refused(rec, device.msm_execute_parts_dev, pre, [(0, dev(3, 4)), (3, t)], **outs)
    refused(rec, device.msm_execute_parts_dev, pre, [(0, dev(3, 4)), (3, dev(2, 4))], buckets=[(0, 1)], **outs)


# ---- the Plonk and Plookup loops ----
def test_vanishing_points_dev(rec):
    ks, sc = limbs(6, 4), [limbs(4, seed=s) for s in range(2, 7)]
    for log_degree in (1, 2):
        n8 = 8 << log_degree
        c, w, s, z, out = dev(6, n8, 4), dev(9, n8, 4), dev(6, n8, 4), dev(n8, 4), dev(n8, 4)
        got = call(rec, ("plk_plonk_vanishing_points_dev", 1, log_degree, P(c), P(w), P(s), P(z), H(ks), H(sc[0]), H(sc[1]), H(sc[2]), H(sc[3]), H(sc[4]),
                         P(out), STREAM), device.vanishing_points_dev, 1, log_degree, c, w, s, z, ks.tolist(), *sc, out=out)
        assert got is out
    good = [dev(6, 16, 4), dev(9, 16, 4), dev(6, 16, 4), dev(16, 4)]
    for k, rows in enumerate((6, 9, 6, 1)):
        for t in bad_tensors(rows, 16, 4) + [dev(rows, 15, 4)]:
            refused(rec, device.vanishing_points_dev, 1, 1, *(good[:k] + [t] + good[k + 1:]), ks, *sc, out=dev(16, 4))


def _status_cases(words):
    """(status argument, pointer the call gets, whether the wrapper returns it)"""
    t = dev(words, dtype=torch.int32)
    return ((None, NULL, False), (False, NULL, False), (t, P(t), True))


def _bad_status(words):
    return bad_tensors(words, dtype=torch.int32, wrong_dtype=torch.int64) + [dev(words + 1, dtype=torch.int32), dev(words - 1, dtype=torch.int32)]


def test_permutation_polynomial_dev(rec):
    ks, beta, gamma = limbs(6, 4), limbs(4, seed=2), limbs(4, seed=3)
    for log_degree, rows, stride, (status, sp, returned) in itertools.product((1, 2), (6, 9), (1, 8), _status_cases(2)):
        n = 1 << log_degree
        w, s, out = dev(rows, n, 4), dev(6, n * stride, 4), dev(n, 4)
        got = call(rec, ("plk_plonk_permutation_z_dev", 0, log_degree, P(w), P(s), stride, H(ks), H(beta), H(gamma), P(out), sp, STREAM),
                   device.permutation_polynomial_dev, 0, log_degree, w, s, ks, beta, gamma, sigma_stride=stride, out=out, status=status)
        assert (got[0] is out and got[1] is status) if returned else got is out
    args = lambda w=None, s=None: (0, 1, dev(6, 2, 4) if w is None else w, dev(6, 16, 4) if s is None else s, ks, beta, gamma)
    for w in bad_tensors(6, 2, 4) + [dev(5, 2, 4), dev(49)]:
        refused(rec, device.permutation_polynomial_dev, *args(w=w), out=dev(2, 4))
    for s in bad_tensors(6, 16, 4) + [dev(6, 2, 4)]:
        refused(rec, device.permutation_polynomial_dev, *args(s=s), out=dev(2, 4))
    for o in bad_tensors(2, 4) + [dev(3, 4)]:
        refused(rec, device.permutation_polynomial_dev, *args(), out=o)
    for st in _bad_status(2):
        refused(rec, device.permutation_polynomial_dev, *args(), out=dev(2, 4), status=st)
    assert call(rec, ("plk_plonk_permutation_z_dev", 0, 1, ANYPTR, ANYPTR, 8, H(ks), H(beta), H(gamma), ANYPTR, NULL, STREAM),
                device.permutation_polynomial_dev, *args(), out=dev(8)).shape == (8,)  # the numel form: any shape of n * 4 words


def test_sigma_dev(rec):
    ks = limbs(6, 4)
    for log_degree, m, want_sigma, (status, sp, returned) in itertools.product((1, 2), (0, 5), (True, False), _status_cases(3)):
        members, offsets = dev(m, dtype=torch.int32), dev(3, dtype=torch.int32)
        got = call(rec, ("plk_plonk_sigma_dev", log_degree, 1, P(members) if m else NULL, P(offsets), 2, m, H(ks), OUT(0), OUT(1), sp, STREAM),
                   device.sigma_dev, 1, log_degree, members, offsets, ks, want_sigma=want_sigma, status=status)
        n = 1 << log_degree
        assert len(got) == (3 if returned else 2) and (not returned or got[2] is status)
        assert (got[0] is None) == (not want_sigma) and (got[0] is None or (got[0].shape == (6 * n,) and got[0].dtype == torch.int32))
        assert got[1].shape == (6, n, 4) and got[1].dtype == torch.int64
    for t in bad_tensors(4, dtype=torch.int32, wrong_dtype=torch.int64) + [dev(2, 2, dtype=torch.int32)]:
        refused(rec, device.sigma_dev, 1, 1, t, dev(3, dtype=torch.int32), ks)
        refused(rec, device.sigma_dev, 1, 1, dev(5, dtype=torch.int32), t, ks)
    refused(rec, device.sigma_dev, 1, 1, dev(5, dtype=torch.int32), dev(0, dtype=torch.int32), ks)
    for st in _bad_status(3):
        refused(rec, device.sigma_dev, 1, 1, dev(5, dtype=torch.int32), dev(3, dtype=torch.int32), ks, status=st)


def test_plookup_grand_polynomial_dev(rec):
    beta, gamma = limbs(4, seed=2), limbs(4, seed=3)
    for log_size, (status, sp, returned) in itertools.product((1, 2), _status_cases(2)):
        size = 1 << log_size
        f, t, s, out = dev(size, 4), dev(size, 4), dev(2 * size - 1, 4), dev(size, 4)
        got = call(rec, ("plk_plookup_grand_product_dev", log_size, 0, P(f), P(t), P(s), H(beta), H(gamma), P(out), sp, STREAM),
                   device.plookup_grand_polynomial_dev, 0, log_size, f, t, s, beta, gamma, out=out, status=status)
        assert (got[0] is out and got[1] is status) if returned else got is out
    good = [dev(2, 4), dev(2, 4), dev(3, 4)]
    for k, rows in enumerate((2, 2, 3)):
        for x in bad_tensors(rows, 4) + [dev(rows + 1, 4)]:
            refused(rec, device.plookup_grand_polynomial_dev, 0, 1, *(good[:k] + [x] + good[k + 1:]), beta, gamma, out=dev(2, 4))
    for o in bad_tensors(2, 4) + [dev(3, 4)]:
        refused(rec, device.plookup_grand_polynomial_dev, 0, 1, *good, beta, gamma, out=o)
    for st in _bad_status(2):
        refused(rec, device.plookup_grand_polynomial_dev, 0, 1, *good, beta, gamma, out=dev(2, 4), status=st)


def test_plookup_vanishing_values_dev(rec):
    sc = [limbs(4, seed=s) for s in (2, 3, 4)]
    for log_size in (1, 2):
        n4 = 4 << log_size
        v, out = dev(5, n4, 4), dev(n4, 4)
        assert call(rec, ("plk_plookup_vanishing_points_dev", log_size, 0, P(v), H(sc[0]), H(sc[1]), H(sc[2]), P(out), STREAM),
                    device.plookup_vanishing_values_dev, 0, log_size, v, *sc, out=out) is out
    for v in bad_tensors(5, 8, 4) + [dev(4, 8, 4)]:
        refused(rec, device.plookup_vanishing_values_dev, 0, 1, v, *sc, out=dev(8, 4))
    for o in bad_tensors(8, 4) + [dev(7, 4)]:
        refused(rec, device.plookup_vanishing_values_dev, 0, 1, dev(5, 8, 4), *sc, out=o)


def test_plookup_sorted_multiset_dev(rec):
    for log_size, (status, sp, returned) in itertools.product((1, 2), _status_cases(2)):
        size = 1 << log_size
        f, t, out = dev(size, 4), dev(size, 4), dev(2 * size - 1, 4)
        got = call(rec, ("plk_plookup_sorted_multiset_dev", log_size, 0, P(f), P(t), P(out), sp, STREAM),
                   device.plookup_sorted_multiset_dev, 0, log_size, f, t, out=out, status=status)
        assert (got[0] is out and got[1] is status) if returned else got is out
    for x in bad_tensors(2, 4) + [dev(3, 4)]:
        refused(rec, device.plookup_sorted_multiset_dev, 0, 1, x, dev(2, 4), out=dev(3, 4))
        refused(rec, device.plookup_sorted_multiset_dev, 0, 1, dev(2, 4), x, out=dev(3, 4))
    for o in bad_tensors(3, 4) + [dev(4, 4)]:
        refused(rec, device.plookup_sorted_multiset_dev, 0, 1, dev(2, 4), dev(2, 4), out=o)
    for st in _bad_status(2):
        refused(rec, device.plookup_sorted_multiset_dev, 0, 1, dev(2, 4), dev(2, 4), out=dev(3, 4), status=st)


# ---- the opening step ----
def test_powers_dev(rec):
    x, out = limbs(4), dev(5, 4)
    assert call(rec, ("plk_field_powers_dev", 0, H(x), 5, P(out), STREAM), device.powers_dev, 0, x.tolist(), 5, out=out) is out
    for o in bad_tensors(5, 4) + [dev(4, 4), dev(20)]:
        refused(rec, device.powers_dev, 0, x, 5, out=o)


def test_eval_polys_dev(rec):
    for n_points in (1, 8):
        pts = limbs(n_points, 4)
        p0, p1, out = dev(3, 4), dev(0, 4), dev(n_points, 2, 4)
        assert call(rec, ("plk_plonk_eval_polys_dev", 0, 2, PA([p0, None]), H([3, 0]), n_points, H(pts), P(out), STREAM),
                    device.eval_polys_dev, 0, [p0, p1], pts, out=out) is out
        out = dev(n_points, 0, 4)
        assert call(rec, ("plk_plonk_eval_polys_dev", 0, 0, PA([None]), H([]), n_points, H(pts), P(out), STREAM),
                    device.eval_polys_dev, 0, [], pts, out=out) is out
    for p in bad_tensors(3, 4) + [dev(3, 6), dev(12), dev(1, 3, 4)]:
        refused(rec, device.eval_polys_dev, 0, [dev(3, 4), p], limbs(1, 4), out=dev(1, 2, 4))
    for o in bad_tensors(1, 2, 4) + [dev(2, 1, 4), dev(8)]:
        refused(rec, device.eval_polys_dev, 0, [dev(3, 4), dev(3, 4)], limbs(1, 4), out=o)


def test_reduce_polynomials_dev(rec):
    p0, p1, sc, out = dev(3, 4), dev(0, 4), limbs(2, 4), dev(4, 4)
    assert call(rec, ("plk_poly_reduce_dev", 0, 2, PA([p0, None]), H([3, 0]), H(sc), 4, P(out), STREAM),
                device.reduce_polynomials_dev, 0, [p0, p1], sc, 4, out=out) is out
    assert call(rec, ("plk_poly_reduce_dev", 0, 0, PA([None]), H([]), H([]), 4, P(out), STREAM), device.reduce_polynomials_dev, 0, [], [], 4, out=out) is out
    with pytest.raises(AssertionError, match="one scalar per polynomial"):
        device.reduce_polynomials_dev(0, [p0, p1], limbs(3, 4), 4, out=out)
    assert rec.calls == []
    for p in bad_tensors(3, 4) + [dev(3, 6)]:
        refused(rec, device.reduce_polynomials_dev, 0, [p, p1], sc, 4, out=out)
    for o in bad_tensors(4, 4) + [dev(5, 4)]:
        refused(rec, device.reduce_polynomials_dev, 0, [p0, p1], sc, 4, out=o)


def test_build_halo_b_dev_and_halo_s_dev(rec):
    for n_points in (1, 8):
        pts, v, out = limbs(n_points, 4), limbs(4, seed=5), dev(4, 4)
        assert call(rec, ("plk_halo_build_b_dev", 0, n_points, H(pts), H(v), 4, P(out), STREAM), device.build_halo_b_dev, 0, pts, v, 4, out=out) is out
    refused(rec, device.build_halo_b_dev, 0, limbs(1, 4), limbs(4), 4, out=dev(3, 4))
    for k in (1, 2):
        us, out = limbs(k, 4), dev(1 << k, 4)
        assert call(rec, ("plk_halo_s_dev", 0, k, H(us), P(out), STREAM), device.halo_s_dev, 0, us, out=out) is out
    for o in bad_tensors(4, 4) + [dev(2, 4)]:
        refused(rec, device.halo_s_dev, 0, limbs(2, 4), out=o)


# ---- the divisions ----
def test_polynomial_division_dev(rec):
    a, b = dev(40, 4), limbs(3, 4)
    q, r = dev(38, 4), dev(2, 4)
    got = call(rec, ("plk_poly_division_dev", 0, P(a), 40, H(b), 3, P(q), 38, P(r), STREAM), device.polynomial_division_dev, 0, a, b, out=q, rem=r)
    assert got[0] is q and got[1] is r
    q = dev(64, 4)
    call(rec, ("plk_poly_division_dev", 0, P(a), 40, H(b), 3, P(q), 64, P(r), STREAM), device.polynomial_division_dev, 0, a, b, out=q, rem=r)  # q_len from out
    call(rec, ("plk_poly_division_dev", 0, P(a), 40, H(b), 3, P(q), 64, P(r), STREAM), device.polynomial_division_dev, 0, a, b, q_len=64, out=q, rem=r)
    for x in bad_tensors(40, 4) + [dev(40, 6), dev(160)]:
        refused(rec, device.polynomial_division_dev, 0, x, b, out=q, rem=r)
    refused(rec, device.polynomial_division_dev, 0, a, b, q_len=38, out=q, rem=r)
    refused(rec, device.polynomial_division_dev, 0, a, b, out=q, rem=dev(3, 4))


def _own_status_cases():
    """the divisions' own rule: None, or an int32 tensor of at least one word"""
    one, two = dev(1, dtype=torch.int32), dev(2, dtype=torch.int32)
    return ((None, NULL), (one, P(one)), (two, P(two)))


def _bad_own_status():
    return bad_tensors(2, dtype=torch.int32, wrong_dtype=torch.int64) + [cpu(1, dtype=torch.int32), dev(0, dtype=torch.int32)]


def test_polynomial_inv_mod_xn_dev(rec):
    for (lh, n), (status, sp) in itertools.product(((1, 1), (3, 5)), _own_status_cases()):
        h, out = dev(lh, 4), dev(n, 4)
        assert call(rec, ("plk_poly_inv_mod_xn_dev", n, 1, P(h), lh, P(out), sp, STREAM), device.polynomial_inv_mod_xn_dev, 1, h, n, out=out,
                    status=status) is out
    for h in bad_tensors(3, 4) + [dev(3, 6), dev(12)]:
        refused(rec, device.polynomial_inv_mod_xn_dev, 1, h, 5, out=dev(5, 4))
    for o in bad_tensors(5, 4) + [dev(4, 4)]:
        refused(rec, device.polynomial_inv_mod_xn_dev, 1, dev(3, 4), 5, out=o)
    for st in _bad_own_status():
        refused(rec, device.polynomial_inv_mod_xn_dev, 1, dev(3, 4), 5, out=dev(5, 4), status=st)


def test_polynomial_div_rem_dev(rec):
    for status, sp in _own_status_cases():
        a, b, q, r = dev(9, 4), dev(4, 4), dev(6, 4), dev(3, 4)
        got = call(rec, ("plk_poly_div_rem_dev", 9, 1, P(a), P(b), 4, P(q), 6, P(r), sp, STREAM), device.polynomial_div_rem_dev, 1, a, b, out=q, rem=r,
                   status=status)
        assert got[0] is q and got[1] is r
    q = dev(16, 4)
    call(rec, ("plk_poly_div_rem_dev", 9, 1, P(a), P(b), 4, P(q), 16, P(r), NULL, STREAM), device.polynomial_div_rem_dev, 1, a, b, out=q, rem=r)
    for x in bad_tensors(4, 4) + [dev(4, 6), dev(16)]:
        refused(rec, device.polynomial_div_rem_dev, 1, x, b, out=q, rem=r)
        refused(rec, device.polynomial_div_rem_dev, 1, a, x, out=q, rem=r)
    refused(rec, device.polynomial_div_rem_dev, 1, a, b, q_len=6, out=q, rem=r)
    refused(rec, device.polynomial_div_rem_dev, 1, a, b, out=q, rem=dev(4, 4))
    for st in _bad_own_status():
        refused(rec, device.polynomial_div_rem_dev, 1, a, b, out=q, rem=r, status=st)


# ---- the inner-product argument ----
def test_inner_product_dev_and_fold_slices_dev(rec):
    for (field, L), n, dtype in itertools.product(FIELDS, (1, 2), (torch.int64, torch.uint8)):  # the dtype is not looked at
        a, b = dev(n, L, dtype=dtype), dev(n, L, dtype=dtype)
        got = call(rec, ("plk_field_inner_product_dev", field, P(a), P(b), n, OUT(), STREAM), device.inner_product_dev, field, a, b)
        assert got.shape == (1, L) and got.dtype == torch.int64
        sl, sh = limbs(L, seed=2), limbs(L, seed=3)
        got = call(rec, ("plk_field_fold_slices_dev", field, P(a), P(b), H(sl), H(sh), n, OUT(), STREAM), device.fold_slices_dev, field, a, b, sl, sh)
        assert got.shape == a.shape and got.dtype == dtype
    for x in (cpu(2, 4), strided(2, 4), dev(3, 4), dev(2, 6)):
        for args in ((dev(2, 4), x), (x, dev(2, 4))):
            refused(rec, device.inner_product_dev, 0, *args)
            refused(rec, device.fold_slices_dev, 0, *args, limbs(4), limbs(4))


def test_fold_generators_dev(rec):
    sl, sh = limbs(4, seed=2), limbs(4, seed=3)
    for (curve, L), m, dtype, flags in itertools.product(CURVES, (1, 2), (torch.int64, torch.uint8), (False, True)):
        lo, hi = dev(m, 2, L, dtype=dtype), dev(m, 2, L, dtype=dtype)
        lz, hz = (dev(m, dtype=torch.uint8), dev(m, dtype=torch.uint8)) if flags else (None, None)
        got = call(rec, ("plk_curve_fold_pairs_dev", curve, m, P(lo), P(lz) if flags else NULL, P(hi), P(hz) if flags else NULL, H(sl), H(sh), OUT(0), OUT(1),
                         STREAM), device.fold_generators_dev, curve, lo, hi, sl, sh, lo_zero=lz, hi_zero=hz)
        assert got[0].shape == (m, 2, L) and got[0].dtype == dtype and got[1].shape == (m,) and got[1].dtype == torch.uint8
    for x in (cpu(2, 2, 4), strided(2, 2, 4), dev(3, 2, 4)):
        refused(rec, device.fold_generators_dev, 0, dev(2, 2, 4), x, sl, sh)
        refused(rec, device.fold_generators_dev, 0, x, dev(2, 2, 4), sl, sh)


def test_fold_generators_multi_dev(rec):
    for (curve, L), (n, log_inputs), dtype, flags in itertools.product(CURVES, ((4, 1), (4, 2), (8, 2)), (torch.int64, torch.uint8), (False, True)):
        g, s = dev(n, 2, L, dtype=dtype), dev(1 << log_inputs, 4, dtype=dtype)
        gz = dev(n, dtype=torch.uint8) if flags else None
        got = call(rec, ("plk_curve_fold_multi_dev", curve, n >> log_inputs, log_inputs, P(g), P(gz) if flags else NULL, P(s), OUT(0), OUT(1), STREAM),
                   device.fold_generators_multi_dev, curve, g, s, log_inputs, g_zero=gz)
        assert got[0].shape == (n >> log_inputs, 2, L) and got[0].dtype == dtype and got[1].shape == (n >> log_inputs,) and got[1].dtype == torch.uint8
    for g in (cpu(4, 2, 4), strided(4, 2, 4), dev(3, 2, 4)):
        refused(rec, device.fold_generators_multi_dev, 0, g, dev(2, 4), 1)
    for s in (cpu(2, 4), strided(2, 4), dev(4, 4)):
        refused(rec, device.fold_generators_multi_dev, 0, dev(4, 2, 4), s, 1)


def test_halo_argument(rec):
    for (curve, L), n, flags in itertools.product(CURVES, (1, 8), (False, True)):
        a, b, g = dev(n, 4), dev(n, 4), dev(n, 2, L)
        gz = dev(n, dtype=torch.uint8) if flags else None
        zp = P(gz) if flags else NULL
        h, u, xs = limbs(2, L, seed=2), limbs(2, L, seed=3), limbs(4, seed=4)
        ref = REF(ctypes.c_void_p)
        arg = call(rec, ("plk_halo_begin_dev", curve, n, P(a), P(b), P(g), zp, H(h), H(u), 3, STREAM, ref),
                   device.HaloArgument, curve, a, b, g, h.tolist(), u, g_zero=gz, freeze_log=3)
        assert (arg.curve, arg.L) == (curve, L) and not hasattr(arg, "_tables") and isinstance(arg._ctx, ctypes.c_void_p)
        tables = SimpleNamespace(_ctx=TABLES)
        arg = call(rec, ("plk_halo_begin_tabled_dev", curve, n, P(a), P(b), P(g), zp, TABLES, H(h), H(u), NO, NO, NULL, 3, 2, STREAM, ref),
                   device.HaloArgument, curve, a, b, g, h, u, g_zero=gz, freeze_log=3, tables=tables, lead_rounds=2)
        assert arg._tables is tables
        call(rec, ("plk_halo_begin_tabled_dev", curve, n, P(a), P(b), P(g), zp, TABLES, H(h), H(u), NO, NO, NULL, 0, 2, STREAM, ref),
             device.HaloArgument, curve, a, b, g, h, u, g_zero=gz, tables=tables, lead_rounds=2, h_index=n, u_index=n + 1)  # no scalar: not inside
        arg = call(rec, ("plk_halo_begin_tabled_dev", curve, n, P(a), P(b), P(g), zp, TABLES, H(h), H(u), n, n + 1, H(xs), 0, 2, STREAM, ref),
                   device.HaloArgument, curve, a, b, g, h, u, g_zero=gz, tables=tables, lead_rounds=2, h_index=n, u_index=n + 1, u_prime_scalar=xs)
        assert arg._tables is tables
    a, b, g, h, u = dev(2, 4), dev(2, 4), dev(2, 2, 4), limbs(2, 4), limbs(2, 4)
    for x in bad_tensors(2, 4) + [dev(3, 4)]:
        refused(rec, device.HaloArgument, 0, x, b, g, h, u)
        refused(rec, device.HaloArgument, 0, a, x, g, h, u)
    for x in bad_tensors(2, 2, 4) + [dev(3, 2, 4)]:
        refused(rec, device.HaloArgument, 0, a, b, x, h, u)


def test_halo_argument_rounds_and_lifetime(rec):
    arg = call(rec, ("plk_halo_begin_dev", 0, 2, ANYPTR, ANYPTR, ANYPTR, NULL, ANYPTR, ANYPTR, 0, STREAM, REF(ctypes.c_void_p)),
               device.HaloArgument, 0, dev(2, 4), dev(2, 4), dev(2, 2, 4), limbs(2, 4), limbs(2, 4))
    arg.free()  # a context that was never handed out is not freed
    assert rec.calls == []
    arg._ctx = CTX
    assert call(rec, ("plk_halo_len", CTX), len, arg) == 0 and call(rec, ("plk_halo_frozen", CTX), lambda: arg.frozen) is False
    lb, rb = limbs(4, seed=2), limbs(4, seed=3)
    lr, z = call(rec, ("plk_halo_round_lr", CTX, H(lb), H(rb), OUT(0), OUT(1)), arg.round_lr, lb, rb.tolist())
    assert lr.shape == (2, 2, 4) and lr.dtype == np.uint64 and z.shape == (2,) and z.dtype == np.uint8
    call(rec, ("plk_halo_round_fold", CTX, H(lb), H(rb)), arg.round_fold, lb, rb)
    got = call(rec, [("plk_halo_len", CTX), ("plk_halo_read", CTX, OUT(0), OUT(1), NULL, NULL)], arg.read, with_g=False)
    assert len(got) == 2
    got = call(rec, [("plk_halo_len", CTX), ("plk_halo_read", CTX, OUT(0), OUT(1), OUT(2), OUT(3))], arg.read)
    assert len(got) == 4 and got[2].shape == (0, 2, 4) and got[3].dtype == np.uint8
    call(rec, ("plk_halo_free", CTX), arg.free)
    assert arg._ctx is None
    arg.free()
    del arg
    assert rec.calls == []


# ---- Rescue ----
def test_rescue_dev(rec):
    for (field, L), n in itertools.product(FIELDS, (1, 2)):
        ctx = SimpleNamespace(field=field, width=4, handle=HANDLE)
        states, out = dev(n, 4, L), dev(n, 4, L)
        assert call(rec, ("plk_rescue_permutation_dev", n, HANDLE, P(states), P(out), STREAM), device.rescue_permutation_dev, ctx, states, out=out) is out
        assert call(rec, ("plk_rescue_permutation_dev", n, HANDLE, P(states), P(states), STREAM), device.rescue_permutation_dev, ctx, states,
                    out=states) is states
        for n_inputs in (0, 3):
            inputs, out = dev(n, n_inputs, L), dev(n, 2, L)
            assert call(rec, ("plk_rescue_sponge_dev", n, HANDLE, n_inputs, P(inputs), 2, P(out), STREAM), device.rescue_sponge_dev, ctx, inputs, 2,
                        out=out) is out
        x, out = dev(n, L), dev(n, L)
        assert call(rec, ("plk_field_kth_root_dev", n, field, 5, P(x), P(out), STREAM), device.kth_root_dev, field, x, 5, out=out) is out
    ctx = SimpleNamespace(field=0, width=4, handle=HANDLE)
    for s in bad_tensors(2, 4, 4) + [dev(2, 3, 4), dev(2, 4, 6), dev(2, 16)]:
        refused(rec, device.rescue_permutation_dev, ctx, s, out=dev(2, 4, 4))
    for o in bad_tensors(2, 4, 4) + [dev(3, 4, 4), dev(32)]:
        refused(rec, device.rescue_permutation_dev, ctx, dev(2, 4, 4), out=o)
    for i in bad_tensors(2, 3, 4) + [dev(2, 3, 6), dev(6, 4)]:
        refused(rec, device.rescue_sponge_dev, ctx, i, 2, out=dev(2, 2, 4))
    for o in bad_tensors(2, 2, 4) + [dev(2, 3, 4), dev(16)]:
        refused(rec, device.rescue_sponge_dev, ctx, dev(2, 3, 4), 2, out=o)
    for x in bad_tensors(2, 4) + [dev(2, 6)]:
        refused(rec, device.kth_root_dev, 0, x, 5, out=dev(2, 4))
    for o in bad_tensors(2, 4) + [dev(3, 4), dev(8)]:
        refused(rec, device.kth_root_dev, 0, dev(2, 4), 5, out=o)


def test_rescue_hash_to_curve_dev(rec):
    for (curve, L), count in itertools.product(CURVES, (1, 2)):
        ctx = SimpleNamespace(handle=HANDLE)
        out, seeds = dev(count, 2, L), dev(count, L)
        assert call(rec, ("plk_rescue_hash_to_curve_dev", count, HANDLE, curve, 9, P(out), STREAM), device.rescue_hash_to_curve_dev, ctx, curve, count,
                    seed_start=9, out=out) is out
        assert call(rec, ("plk_rescue_hash_field_to_curve_dev", count, HANDLE, curve, P(seeds), P(out), STREAM), device.rescue_hash_field_to_curve_dev,
                    ctx, curve, seeds, out=out) is out
    ctx = SimpleNamespace(handle=HANDLE)
    for o in bad_tensors(2, 2, 4) + [dev(3, 2, 4), dev(16)]:
        refused(rec, device.rescue_hash_to_curve_dev, ctx, 0, 2, out=o)
        refused(rec, device.rescue_hash_field_to_curve_dev, ctx, 0, dev(2, 4), out=o)
    refused(rec, device.rescue_hash_to_curve_dev, ctx, 0, 2, device="cpu")  # a fresh out that is not on a GPU
    for s in bad_tensors(2, 4) + [dev(2, 6), dev(8)]:
        refused(rec, device.rescue_hash_field_to_curve_dev, ctx, 0, s, out=dev(2, 2, 4))


# ---- a point times a scalar of its own ----
def test_scalar_mul_dev_and_halo_n(rec):
    for (curve, L), (ns, npts), flags in itertools.product(CURVES, ((1, 1), (8, 8), (1, 8), (8, 1)), (False, True)):
        count = max(ns, npts)
        s, p, out, oz = dev(ns, 4), dev(npts, 2, L), dev(count, 2, L), dev(count, dtype=torch.uint8)
        zero = dev(npts, dtype=torch.uint8) if flags else None
        zp = P(zero) if flags else NULL
        got = call(rec, ("plk_curve_scalar_mul_dev", count, curve, ns, P(s), npts, P(p), zp, P(out), P(oz), STREAM), device.scalar_mul_dev, curve, s, p,
                   zero=zero, out=out, out_zero=oz)
        assert got[0] is out and got[1] is oz
        got = call(rec, ("plk_halo_n_mul_dev", count, curve, 100, ns, P(s), npts, P(p), zp, P(out), P(oz), STREAM), device.halo_n_mul_dev, curve, s, p,
                   zero=zero, security_bits=100, out=out, out_zero=oz)
        assert got[0] is out and got[1] is oz
        assert call(rec, ("plk_halo_n_dev", ns, curve, 128, P(s), P(s), STREAM), device.halo_n_dev, curve, s, out=s) is s
    good = lambda **kw: dict(dict(scalars=dev(2, 4), points=dev(2, 2, 4), zero=dev(2, dtype=torch.uint8), out=dev(2, 2, 4), out_zero=dev(2, dtype=torch.uint8)), **kw)
    faults = [("scalars", t) for t in bad_tensors(2, 4) + [dev(2, 6)]] + [("points", t) for t in bad_tensors(2, 2, 4) + [dev(2, 2, 6), dev(2, 3, 4)]]
    faults += [("zero", t) for t in bad_tensors(2, dtype=torch.uint8) + [dev(3, dtype=torch.uint8)]]
    faults += [("out", t) for t in bad_tensors(2, 2, 4) + [dev(3, 2, 4)]] + [("out_zero", t) for t in bad_tensors(2, dtype=torch.uint8) + [dev(3, dtype=torch.uint8)]]
    for name, t in faults:
        refused(rec, device.scalar_mul_dev, 0, **good(**{name: t}))
        refused(rec, device.halo_n_mul_dev, 0, **good(**{name: t}))
    for s in bad_tensors(2, 4) + [dev(2, 6)]:
        refused(rec, device.halo_n_dev, 0, s, out=dev(2, 4))
    for o in bad_tensors(2, 4) + [dev(3, 4), dev(8)]:
        refused(rec, device.halo_n_dev, 0, dev(2, 4), out=o)
