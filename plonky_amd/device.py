"""Device-resident entry points (torch tensors as HBM buffers, raw pointers into the C ABI).

PyTorch is plumbing here: it owns device memory and streams; every computation is a call into
libplonky_hip.so.  Tensors are int64 views of the reference's u64 limbs, shape (..., L).
"""
import ctypes
import math

import numpy as np
import torch

from . import api as _api, lib as _lib
from .api import _CURVE_LIMBS, _FIELD_LIMBS, MsmPrecomputation, _call, _ptr as _hp, _u64, log2_strict


# ---- the marshalling layer: every wrapper below is a check, _out_tensor and one call ----
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dp(t):
    """the device pointer of a tensor; None for None"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dps(tensors, count):
    """a ctypes array of `count` device pointers (None: a null entry)"""
    return (ctypes.c_void_p * count)(*map(_dp, tensors))


def _check(t, dtype=torch.int64, shape=None, last=None, numel=None):
    """The one tensor check: on the device, contiguous, of that dtype (None: not looked at) and, where given, of that shape (a None
    extent is free), with those trailing extents, of that many elements."""
    assert t.is_cuda and t.is_contiguous() and (dtype is None or t.dtype == dtype)
    assert shape is None or (t.dim() == len(shape) and all(w is None or w == s for w, s in zip(shape, t.shape)))
    assert last is None or tuple(t.shape[-len(last):]) == tuple(last)
    assert numel is None or t.numel() == numel


def _out_tensor(out, shape, device, dtype=torch.int64, check="shape"):
    """An `out=` parameter: a fresh tensor when None; the caller's is checked for its exact shape, for its numel alone
    (check="numel") or not at all (check=None: the wrappers that take it as it is)."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if check == "shape":
        _check(out, dtype, shape=shape)
    elif check == "numel":
        _check(out, dtype, numel=math.prod(shape))
    return out


def _status(status, words, device):
    """A `status=` parameter: None or False - no status words; True - a fresh tensor; or the caller's int32 tensor of exactly `words`
    -> (the tensor or None, its pointer or None)."""
    if status is None or status is False:
        return None, None
    if status is True:
        status = torch.empty(words, dtype=torch.int32, device=device)
    _check(status, torch.int32, numel=words)
    return status, _dp(status)


def init(device_index=None):
    if device_index is None:
        device_index = torch.cuda.current_device()
    torch.cuda.set_device(device_index)
    _lib.check(_lib.load().plk_init(int(device_index)))
    return device_index


def to_device(arr, device="cuda"):
    return torch.from_numpy(_u64(arr).view(np.int64)).to(device)


def to_host(t):
    return t.detach().cpu().numpy().view(np.uint64)


def ntt_dev(field, x, inverse=False, out=None):
    """x: (batch, n, L) or (n, L) int64 CUDA tensor, L = 4 (6 for Bls12377Base); returns the transforms (natural order)."""
    L = _FIELD_LIMBS[field]
    _check(x, last=(L,))
    n = x.shape[-2]
    batch = x.numel() // (n * L)
    log_n = log2_strict(n)
    out = _out_tensor(out, x.shape, x.device, check=None)
    _lib.check(_lib.load().plk_ntt_dev(field, log_n, 1 if inverse else 0, batch, _dp(x), _dp(out), _stream()))
    return out


def ntt_padded_dev(field, x, log_n, out=None):
    """polynomials_to_values_padded on device-resident coefficients: x (batch, len, 4) or (len, 4) with
    len <= 2^log_n; returns (batch, 2^log_n, 4) evaluations.  The zero padding is never stored.  (6 limbs for Bls12377Base.)"""
    L = _FIELD_LIMBS[field]
    _check(x, last=(L,))
    length = x.shape[-2]
    batch = math.prod(x.shape[:-2])  # independent of the length: (B, 0, 4) is B zero polynomials, every output is written
    out = _out_tensor(out, x.shape[:-2] + (1 << log_n, L), x.device, check=None)
    _lib.check(_lib.load().plk_ntt_padded_dev(field, log_n, batch, _dp(x), length, length, _dp(out), _stream()))
    return out


def divide_by_z_h_dev(field, coeffs, n, out=None):
    """Polynomial::divide_by_z_h on a device-resident (len, 4) coefficient tensor; returns a view of the
    2^ceil(log2(degree + 1)) result coefficients (one stream synchronisation: the degree picks the domain)."""
    _check(coeffs, last=(4,))
    length = coeffs.shape[0]
    cap = max(length, 1 << max(0, (length - 1).bit_length()))
    out = _out_tensor(out, (cap, 4), coeffs.device, check=None)
    assert out.shape[0] >= cap
    out_len = ctypes.c_size_t(0)
    _lib.check(_lib.load().plk_poly_divide_by_z_h_dev(field, _dp(coeffs), length, n, _dp(out), out.shape[0], ctypes.byref(out_len), _stream()))
    return out[: out_len.value]


def poly_mul_dev(field, a, b):
    """Polynomial::mul on device-resident coefficient tensors."""
    for t in (a, b):
        _check(t, last=(4,))
    cap = 1 << max(0, (a.shape[0] + b.shape[0] - 1).bit_length())
    out = torch.empty((cap, 4), dtype=torch.int64, device=a.device)
    out_len = ctypes.c_size_t(0)
    _lib.check(_lib.load().plk_poly_mul_dev(field, _dp(a), a.shape[0], _dp(b), b.shape[0], _dp(out), cap, ctypes.byref(out_len), _stream()))
    return out[: out_len.value]


def gen_bases_dev(curve, n, g0_xy, d_xy, first=0, device="cuda"):
    """B_i = G0 + (first + i) D on the device: (n, 2, L) int64 tensor."""
    out = torch.empty((n, 2, _CURVE_LIMBS[curve]), dtype=torch.int64, device=device)
    _lib.check(_lib.load().plk_curve_gen_bases_dev(curve, n, first, _hp(_u64(g0_xy)), _hp(_u64(d_xy)), _dp(out), _stream()))
    return out


def hash_to_curve_dev(curve, count, seed_start=0, seeds=None, out=None, device="cuda"):
    """The Pedersen generators on the device (hash_to_curve.rs:53-76): the points of the integers seed_start .. seed_start + count - 1,
    or, with seeds ((count, L) int64 CUDA tensor, Montgomery form), of those base-field elements.  (count, 2, L) int64 tensor that
    msm_precompute_dev takes as it is."""
    L = _CURVE_LIMBS[curve]
    if seeds is not None:
        _check(seeds, shape=(count, L))
        device = seeds.device
    out = _out_tensor(out, (count, 2, L), device)
    assert out.is_cuda  # a fresh one too: `device` is the caller's word
    if seeds is None:
        _lib.check(_lib.load().plk_hash_to_curve_dev(count, curve, int(seed_start), _dp(out), _stream()))
    else:
        _lib.check(_lib.load().plk_hash_field_to_curve_dev(count, curve, _dp(seeds), _dp(out), _stream()))
    return out


def msm_precompute_dev(curve, bases, w=11, zero=None, device_window=0, table_free=False):
    """bases: (n, 2, L) int64 CUDA tensor.  table_free: no window tables (generators used once or a few times)."""
    _check(bases)
    n = bases.shape[0]
    ctx = ctypes.c_void_p()
    _lib.check(_lib.load().plk_msm_precompute_dev_ex(curve, n, _dp(bases), _dp(zero), device_window, 1 if table_free else 0, _stream(), ctypes.byref(ctx)))
    return MsmPrecomputation(curve, ctx, n, w)


def msm_execute_dev(pre, scalars, out_xy=None, out_zero=None, projective=False):
    """scalars: (batch, n, 4) or (n, 4) int64 CUDA tensor.  Returns (out_xy (batch, 2, L), out_zero (batch,)) on device.
    projective: the reference's own return type - ProjectivePoints x | y | z, not normalised ((batch, 3, L); plk_msm_execute_projective_dev)."""
    _check(scalars)
    n = scalars.shape[-2]
    assert n == pre.n, "powers_per_generator.len() != scalars.len()"
    batch = scalars.numel() // (n * 4) if n else 1
    L = _CURVE_LIMBS[pre.curve]
    out_xy = _out_tensor(out_xy, (batch, 3 if projective else 2, L), scalars.device, check=None)
    out_zero = _out_tensor(out_zero, (batch,), scalars.device, torch.uint8, check=None)
    assert not projective or out_xy.numel() == batch * 3 * L
    execute = _lib.load().plk_msm_execute_projective_dev if projective else _lib.load().plk_msm_execute_dev
    _lib.check(execute(pre._ctx, batch, _dp(scalars), n, _dp(out_xy), _dp(out_zero), _stream()))
    return out_xy, out_zero


def msm_execute_parts_dev(pre, parts, out_xy=None, out_zero=None, buckets=None):
    """plk_msm_execute_parts_dev: parts = [(first, scalars)] with scalars an (count, 4) int64 CUDA tensor for the generators
    first .. first + count - 1 of `pre` (a tabled precomputation).  One batched call, one shared reduction -> ((batch, 2, L), (batch,)).
    buckets (optional): [(part, parts)] per vector - the vector keeps only the part-th of `parts` ranges of the coarse bucket bins
    (plk_msm_execute_parts_buckets_dev: a rank's BUCKET share of a sharded vector; (0, 1): every bucket)."""
    batch = len(parts)
    dev0 = parts[0][1].device
    out_xy = _out_tensor(out_xy, (batch, 2, _CURVE_LIMBS[pre.curve]), dev0, check=None)
    out_zero = _out_tensor(out_zero, (batch,), dev0, torch.uint8, check=None)
    first = np.array([p[0] for p in parts], dtype=np.uint64)
    count = np.array([p[1].shape[0] for p in parts], dtype=np.uint64)
    for _, t in parts:
        _check(t, last=(4,))
    args = [pre._ctx, batch, _hp(first), _hp(count), _dps([p[1] for p in parts], batch)]
    execute = _lib.load().plk_msm_execute_parts_dev
    if buckets is not None:
        assert len(buckets) == batch
        bp = np.array([b[0] for b in buckets], dtype=np.uint32)
        bn = np.array([b[1] for b in buckets], dtype=np.uint32)
        args += [_hp(bp), _hp(bn)]
        execute = _lib.load().plk_msm_execute_parts_buckets_dev
    _lib.check(execute(*args, _dp(out_xy), _dp(out_zero), _stream()))
    return out_xy, out_zero


def vanishing_points_dev(field, log_degree, constants_8n, wire_values_8n, s_sigma_values_8n, plonk_z_points_8n, k_is, alpha, beta, gamma,
                         inner_zeta, inner_a, out=None):
    """Prover::vanishing_poly's 8n-point loop (plonk.rs:392-453) on device-resident tables: int64 CUDA tensors (6, 8n, 4),
    (9, 8n, 4), (6, 8n, 4), (8n, 4); the scalars are host arrays (4 limbs each; k_is (6, 4))."""
    n8 = 8 << log_degree
    tables = ((constants_8n, 6), (wire_values_8n, 9), (s_sigma_values_8n, 6), (plonk_z_points_8n, 1))
    for t, rows in tables:
        _check(t, numel=rows * n8 * 4)
    out = _out_tensor(out, (n8, 4), constants_8n.device, check=None)
    sc = [_u64(x, 4) for x in (alpha, beta, gamma, inner_zeta, inner_a)]
    _lib.check(_lib.load().plk_plonk_vanishing_points_dev(field, log_degree, *[_dp(t) for t, _ in tables], _hp(_u64(k_is, 6, 4)), *map(_hp, sc),
                                                          _dp(out), _stream()))
    return out


def permutation_polynomial_dev(field, log_degree, wire_values, s_sigma_values, k_is, beta, gamma, sigma_stride=8, out=None, status=None):
    """permutation_polynomial (plonk_util.rs:234-262) on device-resident tables: int64 CUDA tensors wire_values (>= 6, n, 4)
    (wire_values_by_wire_index; rows 0..5 are read) and s_sigma_values (6, n * sigma_stride, 4); the scalars are host arrays
    (k_is (6, 4)).  Returns Z (n, 4); with status=True (or a (2,) int32 CUDA tensor) also the status words, written in stream
    order: [0] zero denominators among rows 0..n-2 (Z unspecified when > 0), [1] 1 iff Z closes the cycle."""
    n = 1 << log_degree
    _check(wire_values)
    assert wire_values.numel() >= 6 * n * 4 and wire_values.numel() % (n * 4) == 0
    _check(s_sigma_values, numel=6 * n * sigma_stride * 4)
    out = _out_tensor(out, (n, 4), wire_values.device, check="numel")
    status, sp = _status(status, 2, wire_values.device)
    ks, b, g = _u64(k_is, 6, 4), _u64(beta, 4), _u64(gamma, 4)
    _lib.check(_lib.load().plk_plonk_permutation_z_dev(field, log_degree, _dp(wire_values), _dp(s_sigma_values), sigma_stride, _hp(ks), _hp(b), _hp(g),
                                                       _dp(out), sp, _stream()))
    return out if status is None else (out, status)


def check_witness_dev(field, log_degree, constants, wires, sigma=None, inner_zeta=None, inner_a=None, constants_stride=8, report=None, row_masks=None,
                      first_terms=None):
    """The witness check (plk_plonk_check_witness_dev, include/plonky_hip_witness.h) on device-resident tables: int64 CUDA tensors
    constants (6, n * constants_stride, 4) - CircuitKey.constants_8n as it is with the default stride 8, the n-point columns with
    stride 1 - and wires (9, n, 4) (wire_values_by_wire_index); sigma (optional) the (6 n,) int32 tensor of sigma_dev /
    CircuitKey.sigma; inner_zeta / inner_a host limbs (both are needed).  Optional outputs, the caller's tensors: row_masks (n,) uint8,
    first_terms (8, 4) int64.  Returns the report, an (8,) int32 CUDA tensor (the caller's, or a fresh one) written in stream order:
    [0] failing rows, [1] the first (-1: none), [2] its mask, [3] routed wires that differ from their copy, [4] the first (-1: none),
    [5] sigma entries >= 6 n, [6], [7] zero; api.WitnessReport decodes its host copy.  A witness that fails is a result, not an error."""
    n = 1 << log_degree
    assert constants_stride in (1, 8), "constants_stride must be 1 or 8"
    assert inner_zeta is not None and inner_a is not None, "inner_zeta and inner_a are needed"
    _check(constants, numel=6 * n * constants_stride * 4)
    _check(wires, numel=9 * n * 4)
    if sigma is not None:
        _check(sigma, torch.int32, numel=6 * n)
    report = _out_tensor(report, (8,), constants.device, torch.int32)
    if row_masks is not None:
        row_masks = _out_tensor(row_masks, (n,), constants.device, torch.uint8)
    if first_terms is not None:
        first_terms = _out_tensor(first_terms, (8, 4), constants.device)
    zeta, a = _u64(inner_zeta, 4), _u64(inner_a, 4)
    _lib.check(_lib.load().plk_plonk_check_witness_dev(log_degree, field, _dp(constants), constants_stride, _dp(wires), _dp(sigma), _hp(zeta), _hp(a), _dp(report),
                                                       _dp(row_masks), _dp(first_terms), _stream()))
    return report


# ---- the copy-constraint permutation and the setup-time half of CircuitBuilder::build ----
def sigma_dev(field, log_degree, members, offsets, k_is, want_sigma=True, status=False):
    """to_sigma (partition.rs:108-136) + sigma_polynomials (plonk_util.rs:264-280) on device-resident partitions: int32 CUDA tensors
    members (M,) (wire ids input * n + gate) and offsets (P + 1,), as api.WirePartitions.to_csr gives them; k_is (6, 4) host limbs.
    Returns (sigma (6 n,) int32 or None, s_sigma (6, n, 4) int64) - s_sigma is what permutation_polynomial_dev takes with
    sigma_stride=1 and ntt_dev with inverse=True; with status=True (or a (3,) int32 CUDA tensor) also the status words, written in
    stream order: [0] routed wires not listed exactly once, [1] non-routed members in a partition of more than one, [2] ids >= 9 n
    (the outputs are unspecified when one is nonzero)."""
    n = 1 << log_degree
    for t in (members, offsets):
        _check(t, torch.int32, shape=(None,))
    assert offsets.numel() >= 1
    sigma = torch.empty(6 * n, dtype=torch.int32, device=members.device) if want_sigma else None
    values = torch.empty((6, n, 4), dtype=torch.int64, device=members.device)
    status, sp = _status(status, 3, members.device)
    ks = _u64(k_is, 6, 4)
    _lib.check(_lib.load().plk_plonk_sigma_dev(log_degree, field, _dp(members if members.numel() else None), _dp(offsets), offsets.numel() - 1,
                                               members.numel(), _hp(ks), _dp(sigma), _dp(values), sp, _stream()))
    return (sigma, values) if status is None else (sigma, values, status)


class CircuitKey:
    """What circuit_key_dev returns: the setup-time fields of Circuit (circuit_builder.rs:1162-1190) that are computed, all on the device."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def circuit_key_dev(curve, log_degree, gate_constants, members, offsets, k_is, w=11):
    """The setup-time half of CircuitBuilder::build (circuit_builder.rs:1118-1160) chained on the device.  gate_constants: (n, 6, 4)
    int64 CUDA tensor, indexed by gate first as the builder holds it; members / offsets / k_is as for sigma_dev, over the curve's
    scalar field.  Returns a CircuitKey with
      pedersen_g (n, 2, L), pedersen_h (2, L), u (2, L)     blake_hash_usize_to_curve of 0..n-1, n, n + 1 (hash_to_curve_dev)
      msm_precomputation                                    over pedersen_g ++ [pedersen_h], the form api.commitment_precompute builds
      constant_polynomials (6, n, 4), constants_8n (6, 8n, 4), c_constants ((6, 2, L), (6,) zero flags)
      sigma (6n,), s_sigma_polynomials (6, n, 4), s_sigma_values_8n (6, 8n, 4), c_s_sigmas ((6, 2, L), (6,))
    The commitments are unblinded (plonk_util.rs:215-231 with blinding off): the scalar of pedersen_h is zero."""
    field = _api.CURVE_SCALAR_FIELD[curve]
    n = 1 << log_degree
    assert gate_constants.is_cuda and gate_constants.dtype == torch.int64 and tuple(gate_constants.shape) == (n, 6, 4)  # any strides: transposed below
    gens = hash_to_curve_dev(curve, n + 2, device=gate_constants.device)
    pre = msm_precompute_dev(curve, gens[: n + 1], w=w)

    def commit(polys):
        return msm_execute_dev(pre, torch.cat([polys, torch.zeros((polys.shape[0], 1, 4), dtype=torch.int64, device=polys.device)], dim=1).contiguous())

    wire_constants = gate_constants.permute(1, 0, 2).contiguous()  # transpose (circuit_builder.rs:1136)
    constant_polynomials = ntt_dev(field, wire_constants, inverse=True)
    constants_8n = ntt_padded_dev(field, constant_polynomials, log_degree + 3)
    c_constants = commit(constant_polynomials)
    sigma, sigma_chunks = sigma_dev(field, log_degree, members, offsets, k_is)
    s_sigma_polynomials = ntt_dev(field, sigma_chunks, inverse=True)
    s_sigma_values_8n = ntt_padded_dev(field, s_sigma_polynomials, log_degree + 3)
    c_s_sigmas = commit(s_sigma_polynomials)
    return CircuitKey(pedersen_g=gens[:n], pedersen_h=gens[n], u=gens[n + 1], msm_precomputation=pre, constant_polynomials=constant_polynomials,
                      constants_8n=constants_8n, c_constants=c_constants, sigma=sigma, s_sigma_polynomials=s_sigma_polynomials,
                      s_sigma_values_8n=s_sigma_values_8n, c_s_sigmas=c_s_sigmas)


# ---- the Plookup prover's two loops on device-resident tables (plookup/src/plookup.rs) ----
def plookup_grand_polynomial_dev(field, log_size, f, t, s, beta, gamma, out=None, status=False):
    """grand_polynomial (plookup.rs:180-202): int64 CUDA tensors f (N, 4) (f_padded; the last row is not read), t (N, 4),
    s (2 N - 1, 4), N = 2^log_size; beta, gamma host limbs.  Returns Z (N, 4); with status=True (or a (2,) int32 CUDA tensor) also the
    status words, written in stream order: [0] zero denominators among rows 0..n-2 (Z unspecified when > 0), [1] 1 iff the product
    over all n rows is 1."""
    size = 1 << log_size
    for x, rows in ((f, size), (t, size), (s, 2 * size - 1)):
        _check(x, numel=rows * 4)
    out = _out_tensor(out, (size, 4), f.device, check="numel")
    status, sp = _status(status, 2, f.device)
    b, g = _u64(beta, 4), _u64(gamma, 4)
    _lib.check(_lib.load().plk_plookup_grand_product_dev(log_size, field, _dp(f), _dp(t), _dp(s), _hp(b), _hp(g), _dp(out), sp, _stream()))
    return out if status is None else (out, status)


def plookup_vanishing_values_dev(field, log_size, values_4n, alpha, beta, gamma, out=None):
    """The 4N-point loop of vanishing_polynomial (plookup.rs:225-269): values_4n an int64 CUDA tensor (5, 4 N, 4), rows z, f, t, h1, h2
    (ntt_padded_dev to log_size + 2); the scalars are host limbs.  Returns (4 N, 4)."""
    n4 = 4 << log_size
    _check(values_4n, numel=5 * n4 * 4)
    out = _out_tensor(out, (n4, 4), values_4n.device, check="numel")
    sc = [_u64(x, 4) for x in (alpha, beta, gamma)]
    _lib.check(_lib.load().plk_plookup_vanishing_points_dev(log_size, field, _dp(values_4n), *map(_hp, sc), _dp(out), _stream()))
    return out


def plookup_sorted_multiset_dev(field, log_size, f, t, out=None, status=False):
    """s of plookup.rs:20-22 (f ++ t in the order of each value's first occurrence in t): int64 CUDA tensors f (N, 4) (f_padded; the
    last row is not read) and t (N, 4), N = 2^log_size.  Returns s (2 N - 1, 4), h1 = s[:N], h2 = s[N - 1:]; with status=True (or a
    (2,) int32 CUDA tensor) also the status words, written in stream order: [0] rows of f whose value is not in t (the reference
    panics; the rows of s beyond the total are zero then), [1] distinct values in t."""
    size = 1 << log_size
    for x in (f, t):
        _check(x, numel=size * 4)
    out = _out_tensor(out, (2 * size - 1, 4), f.device, check="numel")
    status, sp = _status(status, 2, f.device)
    _lib.check(_lib.load().plk_plookup_sorted_multiset_dev(log_size, field, _dp(f), _dp(t), _dp(out), sp, _stream()))
    return out if status is None else (out, status)


# ---- the opening step on device-resident polynomials (plonk.rs:261-308, halo.rs:38-44, 143-155) ----
def _poly_list(polys):
    """list of (len, 4) int64 CUDA tensors -> (ctypes array of device pointers, size_t lengths)"""
    for t in polys:
        _check(t, shape=(None, 4))
    return _dps([t if t.shape[0] else None for t in polys], max(1, len(polys))), np.array([t.shape[0] for t in polys], dtype=np.uint64)


def powers_dev(field, x, n, out=None, device="cuda"):
    """powers (plonk_util.rs:123-133) -> (n, 4) int64 CUDA tensor; x: host limbs."""
    out = _out_tensor(out, (n, 4), device)
    _lib.check(_lib.load().plk_field_powers_dev(field, _hp(_u64(x, 4)), n, _dp(out), _stream()))
    return out


def eval_polys_dev(field, polys, points, out=None):
    """open_all_polynomials (plonk.rs:459-482) for all points at once: polys a list of (len, 4) int64 CUDA tensors (any lengths, the
    same tensor may appear twice), points (n_points, 4) host limbs, 1..8 points -> (n_points, n_polys, 4) CUDA tensor.  Every
    polynomial is read once."""
    ptrs, lens = _poly_list(polys)
    pts = _u64(points, -1, 4)
    out = _out_tensor(out, (pts.shape[0], len(polys), 4), polys[0].device if polys else "cuda")
    _lib.check(_lib.load().plk_plonk_eval_polys_dev(field, len(polys), ptrs, _hp(lens), pts.shape[0], _hp(pts), _dp(out), _stream()))
    return out


def reduce_polynomials_dev(field, polys, scalars, degree, out=None):
    """reduced_coeffs (halo.rs:38-44), the argument's halo_a: sum_i scalars[i] * polys[i], zero-padded to `degree` -> (degree, 4)."""
    ptrs, lens = _poly_list(polys)
    sc = _u64(scalars, -1, 4)
    assert sc.shape[0] == len(polys), "one scalar per polynomial"
    out = _out_tensor(out, (degree, 4), polys[0].device if polys else "cuda")
    _lib.check(_lib.load().plk_poly_reduce_dev(field, len(polys), ptrs, _hp(lens), _hp(sc), degree, _dp(out), _stream()))
    return out


def build_halo_b_dev(field, points, v, degree, out=None, device="cuda"):
    """build_halo_b (halo.rs:143-155), the argument's halo_b: out[j] = sum_k v^k points[k]^j -> (degree, 4)."""
    pts, vs = _u64(points, -1, 4), _u64(v, 4)
    out = _out_tensor(out, (degree, 4), device)
    _lib.check(_lib.load().plk_halo_build_b_dev(field, pts.shape[0], _hp(pts), _hp(vs), degree, _dp(out), _stream()))
    return out


def halo_s_dev(field, us, out=None, device="cuda"):
    """halo_s (plonk_util.rs:311-326) -> (2^k, 4); us: (k, 4) host limbs, none of them zero."""
    u = _u64(us, -1, 4)
    out = _out_tensor(out, (1 << u.shape[0], 4), device)
    _lib.check(_lib.load().plk_halo_s_dev(field, u.shape[0], _hp(u), _dp(out), _stream()))
    return out


# ---- the public-input quotient (plonk.rs:199-235): low-degree polynomial division on device-resident coefficients ----
def polynomial_division_dev(field, a, b, q_len=None, out=None, rem=None):
    """plk_poly_division_dev: a (la, 4) int64 CUDA tensor, b (lb, 4) host limbs with b[lb - 1] != 0 and 1 <= lb - 1 <= 32 < la ->
    (q, rem): q (q_len, 4), the quotient followed by zeros (q_len defaults to la - k), rem (k, 4).  Nothing is synchronised."""
    _check(a, shape=(None, 4))
    bs = _u64(b, -1, 4)
    la, k = a.shape[0], bs.shape[0] - 1
    if q_len is None:
        q_len = out.shape[0] if out is not None else max(la - k, 0)
    out = _out_tensor(out, (q_len, 4), a.device)
    rem = _out_tensor(rem, (max(k, 0), 4), a.device)
    _lib.check(_lib.load().plk_poly_division_dev(field, _dp(a), la, _hp(bs), bs.shape[0], _dp(out), q_len, _dp(rem), _stream()))
    return out, rem


# ---- the series inverse and the division by a divisor of any degree (polydiv_newton.hip): everything stays on the device ----
def _status_ptr(status):
    """the divisions' own status rule: None, or an int32 tensor of at least one word"""
    if status is not None:
        _check(status, torch.int32)
        assert status.numel() >= 1
    return _dp(status)


def polynomial_inv_mod_xn_dev(field, h, n, out=None, status=None):
    """plk_poly_inv_mod_xn_dev: h (lh, 4) int64 CUDA tensor -> g (n, 4) with g h = 1 mod X^n.  status (optional): an int32 CUDA tensor of
    one word; bit 0 is OR-ed in when h[0] == 0 (g is unspecified then).  Nothing is synchronised."""
    _check(h, shape=(None, 4))
    out = _out_tensor(out, (n, 4), h.device)
    _lib.check(_lib.load().plk_poly_inv_mod_xn_dev(n, field, _dp(h), h.shape[0], _dp(out), _status_ptr(status), _stream()))
    return out


def polynomial_div_rem_dev(field, a, b, q_len=None, out=None, rem=None, status=None):
    """plk_poly_div_rem_dev: a (la, 4) and b (lb, 4) int64 CUDA tensors, k = lb - 1 >= 1 of ANY size below la -> (q, rem): q (q_len, 4),
    the quotient followed by zeros (q_len defaults to la - k), rem (k, 4).  status (optional): an int32 CUDA tensor of one word; bit 1 is
    OR-ed in when b[k] == 0 (the outputs are unspecified then).  Nothing is synchronised."""
    for t in (a, b):
        _check(t, shape=(None, 4))
    la, k = a.shape[0], b.shape[0] - 1
    if q_len is None:
        q_len = out.shape[0] if out is not None else max(la - k, 0)
    out = _out_tensor(out, (q_len, 4), a.device)
    rem = _out_tensor(rem, (max(k, 0), 4), a.device)
    _lib.check(_lib.load().plk_poly_div_rem_dev(la, field, _dp(a), _dp(b), b.shape[0], _dp(out), q_len, _dp(rem), _status_ptr(status), _stream()))
    return out, rem


def public_input_quotient_dev(field, wire_polys_no_pis, alpha, roots, degree):
    """The public-input quotient of plonk.rs:199-235: scale_polynomials(wire polynomials without public inputs, alpha, degree) divided
    by prod (X - roots[i]) over the public-input rows -> (quotient padded to `degree`, remainder (k, 4): zero for a valid witness).
    api.powers (the nine powers of alpha, host scalars: a call on the library's own lane) + reduce_polynomials_dev + plk_poly_from_roots + the
    division; the polynomials stay on the device and the caller's stream is never synchronised."""
    pw = _api.powers(field, alpha, len(wire_polys_no_pis))  # host scalars of the reduction: the caller's stream is not touched
    scaled = reduce_polynomials_dev(field, [p[:degree] for p in wire_polys_no_pis], pw, degree)
    return polynomial_division_dev(field, scaled, _api.polynomial_from_roots(field, roots), q_len=degree)


# ---- one round of the inner-product argument (halo.rs:63-124) on device-resident vectors ----
def inner_product_dev(field, a, b):
    """Field::inner_product (field.rs:213-221) -> (1, 4) int64 CUDA tensor."""
    _check(a, None)
    _check(b, None, shape=a.shape)
    out = torch.empty((1, a.shape[-1]), dtype=torch.int64, device=a.device)
    _lib.check(_lib.load().plk_field_inner_product_dev(field, _dp(a), _dp(b), a.shape[0], _dp(out), _stream()))
    return out


def fold_slices_dev(field, lo, hi, scalar_lo, scalar_hi):
    """scalar_lo * lo + scalar_hi * hi (add_slices of scale_slice, halo.rs:117-118)."""
    _check(lo, None)
    _check(hi, None, shape=lo.shape)
    out = torch.empty_like(lo)
    sl, sh = _u64(scalar_lo, lo.shape[-1]), _u64(scalar_hi, lo.shape[-1])
    _lib.check(_lib.load().plk_field_fold_slices_dev(field, _dp(lo), _dp(hi), _hp(sl), _hp(sh), lo.shape[0], _dp(out), _stream()))
    return out


def fold_generators_dev(curve, g_lo, g_hi, scalar_lo, scalar_hi, lo_zero=None, hi_zero=None):
    """G' = [scalar_lo] G_lo + [scalar_hi] G_hi pair by pair (halo.rs:119-123) -> ((m, 2, L), (m,) zero flags) on device."""
    _check(g_lo, None)
    _check(g_hi, None, shape=g_lo.shape)
    m = g_lo.shape[0]
    out = torch.empty_like(g_lo)
    oz = torch.empty((m,), dtype=torch.uint8, device=g_lo.device)
    sl, sh = _u64(scalar_lo, 4), _u64(scalar_hi, 4)
    _lib.check(_lib.load().plk_curve_fold_pairs_dev(curve, m, _dp(g_lo), _dp(lo_zero), _dp(g_hi), _dp(hi_zero), _hp(sl), _hp(sh), _dp(out), _dp(oz),
                                                    _stream()))
    return out, oz


def fold_generators_multi_dev(curve, g, scalars, log_inputs, g_zero=None):
    """out_i = g_i + sum_{t >= 1} [s_t] g_{i + t n_out}, n_out = len(g) >> log_inputs (plk_curve_fold_multi_dev): g (n, 2, L) CUDA,
    scalars (2^log_inputs, 4) CUDA int64 (Montgomery, scalar field) with the scalar of input t at index bitreverse(t)."""
    _check(g, None)
    _check(scalars, None)
    assert scalars.shape[0] == 1 << log_inputs
    n_out = g.shape[0] >> log_inputs
    assert n_out << log_inputs == g.shape[0]
    out = torch.empty((n_out,) + tuple(g.shape[1:]), dtype=g.dtype, device=g.device)
    oz = torch.empty((n_out,), dtype=torch.uint8, device=g.device)
    _lib.check(_lib.load().plk_curve_fold_multi_dev(curve, n_out, log_inputs, _dp(g), _dp(g_zero), _dp(scalars), _dp(out), _dp(oz), _stream()))
    return out, oz


def halo_round_lr_dev(curve, halo_a, halo_b, halo_g, pedersen_h, u_prime, l_blinding, r_blinding, g_zero=None):
    """L_j = <a_lo, G_hi> + [l_j] H + [<a_lo, b_hi>] U',  R_j = <a_hi, G_lo> + [r_j] H + [<a_hi, b_lo>] U' (halo.rs:86-93).
    halo_a / halo_b: (n, 4) scalars, halo_g: (n, 2, L) affine generators (g_zero: (n,) identity flags or None); pedersen_h /
    u_prime: (2, L) affine host points; the blinding factors are host scalars.  The msm_parallel, the blinding term and the
    inner-product term are ONE table-free MSM over [G_half..., H, U'] each.  Returns ((2, 2, L), (2,)): L_j then R_j, affine."""
    n = halo_a.shape[0]
    m = n // 2
    sf = _api.CURVE_SCALAR_FIELD[curve]
    L = _CURVE_LIMBS[curve]
    extra = to_device(np.stack([_u64(pedersen_h, 2, L), _u64(u_prime, 2, L)]))
    # L_j and R_j are independent and, below 2^16 points, pure latency (the window-doubling chain of a table-free MSM):
    # they run on two streams
    main = torch.cuda.current_stream()
    side = _side_stream(halo_a.device)
    side.wait_stream(main)
    outs, zeros = [], []
    for k, (a_half, b_half, g_half, gz, blind) in enumerate(((halo_a[:m], halo_b[m:], halo_g[m:], None if g_zero is None else g_zero[m:], l_blinding),
                                                             (halo_a[m:], halo_b[:m], halo_g[:m], None if g_zero is None else g_zero[:m], r_blinding))):
        st = main if k == 0 else side
        with torch.cuda.stream(st):
            ip = inner_product_dev(sf, a_half.contiguous(), b_half.contiguous())
            scal = torch.cat([a_half, to_device(_u64(blind, 1, 4)), ip], dim=0).contiguous()
            bases = torch.cat([g_half, extra], dim=0).contiguous()
            zf = None
            if gz is not None:
                zf = torch.cat([gz, torch.zeros(2, dtype=torch.uint8, device=gz.device)]).contiguous()
            pre = msm_precompute_dev(curve, bases, zero=zf, table_free=True)
            xy, z = msm_execute_dev(pre, scal)
            pre.free()  # a table-free context hands its memory back in stream order: no synchronisation
            if st is side:
                for t in (halo_a, halo_b, halo_g, extra, g_zero):
                    if t is not None:
                        t.record_stream(side)
                for t in (xy, z):  # allocated on the side stream, read by torch.stack on the main stream below
                    t.record_stream(main)
        outs.append(xy[0])
        zeros.append(z[0])
    main.wait_stream(side)
    return torch.stack(outs), torch.stack(zeros)


_SIDE_STREAMS = {}


def _side_stream(device):
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=key)
    return _SIDE_STREAMS[key]


def halo_round_fold_dev(curve, halo_a, halo_b, halo_g, u_j, u_j_inv, g_zero=None):
    """halo_a' = u^-1 a_hi + u a_lo, halo_b' = u^-1 b_lo + u b_hi, G' = [u^-1] G_lo + [u] G_hi (halo.rs:117-123)."""
    m = halo_a.shape[0] // 2
    sf = _api.CURVE_SCALAR_FIELD[curve]
    a2 = fold_slices_dev(sf, halo_a[m:].contiguous(), halo_a[:m].contiguous(), u_j_inv, u_j)
    b2 = fold_slices_dev(sf, halo_b[:m].contiguous(), halo_b[m:].contiguous(), u_j_inv, u_j)
    g2, gz2 = fold_generators_dev(curve, halo_g[:m].contiguous(), halo_g[m:].contiguous(), u_j_inv, u_j,
                                  None if g_zero is None else g_zero[:m].contiguous(), None if g_zero is None else g_zero[m:].contiguous())
    return a2, b2, g2, gz2


class HaloArgument:
    """One inner-product argument (halo.rs:63-124) behind the C ABI (plk_halo_*): halo_a / halo_b / halo_g are copied into a
    library context and stay in HBM for the log2(n) rounds; per round the caller - who owns the transcript and the RNG -
    calls round_lr(l_j, r_j) (possibly again, halo.rs:83-114) and round_fold(u_j, u_j^-1).  halo_a / halo_b: (n, 4) int64
    CUDA tensors (Montgomery, scalar field); halo_g: (n, 2, L); g_zero: (n,) uint8 or None; pedersen_h / u_prime: (2, L) host."""

    def __init__(self, curve, halo_a, halo_b, halo_g, pedersen_h, u_prime, g_zero=None, freeze_log=0, tables=None, lead_rounds=0, h_index=None, u_index=None,
                 u_prime_scalar=None):
        for t in (halo_a, halo_b, halo_g):
            _check(t)
        n = halo_a.shape[0]
        assert halo_b.shape[0] == n and halo_g.shape[0] == n
        self.curve, self.L = curve, _CURVE_LIMBS[curve]
        h, u = _u64(pedersen_h, 2, self.L), _u64(u_prime, 2, self.L)
        ctx = ctypes.c_void_p()
        vectors = (curve, n, _dp(halo_a), _dp(halo_b), _dp(halo_g), _dp(g_zero))
        if tables is not None:
            # tables: the MsmPrecomputation (msm_precompute_dev) of pedersen_g the caller commits with - the first rounds run over it
            # h_index / u_index / u_prime_scalar: pedersen_h and the fixed generator U inside those tables, u_prime = [u_prime_scalar] U
            self._tables = tables  # must outlive the lead rounds
            NO = ctypes.c_size_t(-1).value
            inside = u_prime_scalar is not None and h_index is not None and u_index is not None
            xs = _u64(u_prime_scalar, 4) if inside else None
            _lib.check(_lib.load().plk_halo_begin_tabled_dev(*vectors, tables._ctx, _hp(h), _hp(u), h_index if inside else NO, u_index if inside else NO,
                                                             _hp(xs), freeze_log, lead_rounds, _stream(), ctypes.byref(ctx)))
        else:
            _lib.check(_lib.load().plk_halo_begin_dev(*vectors, _hp(h), _hp(u), freeze_log, _stream(), ctypes.byref(ctx)))
        self._ctx = ctx

    def __len__(self):
        return int(_lib.load().plk_halo_len(self._ctx))

    @property
    def frozen(self):
        return bool(_lib.load().plk_halo_frozen(self._ctx))

    def round_lr(self, l_blinding, r_blinding):
        """(L_j, R_j) as a (2, 2, L) uint64 array + (2,) identity flags, on the host (the transcript's input)."""
        lr = np.empty((2, 2, self.L), dtype=np.uint64)
        z = np.zeros(2, dtype=np.uint8)
        lb, rb = _u64(l_blinding, 4), _u64(r_blinding, 4)
        _lib.check(_lib.load().plk_halo_round_lr(self._ctx, _hp(lb), _hp(rb), _hp(lr), _hp(z)))
        return lr, z

    def round_fold(self, u_j, u_j_inv):
        u, ui = _u64(u_j, 4), _u64(u_j_inv, 4)
        _lib.check(_lib.load().plk_halo_round_fold(self._ctx, _hp(u), _hp(ui)))

    def read(self, with_g=True):
        """(halo_a, halo_b[, halo_g, g_zero]) on the host; halo_g of frozen generators exists at length 1 only."""
        n = len(self)
        a, b = np.empty((n, 4), dtype=np.uint64), np.empty((n, 4), dtype=np.uint64)
        if not with_g:
            _lib.check(_lib.load().plk_halo_read(self._ctx, _hp(a), _hp(b), None, None))
            return a, b
        g, gz = np.empty((n, 2, self.L), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
        _lib.check(_lib.load().plk_halo_read(self._ctx, _hp(a), _hp(b), _hp(g), _hp(gz)))
        return a, b, g, gz

    def free(self):
        if self._ctx:
            _lib.load().plk_halo_free(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- Rescue on device-resident tensors (rescue.rs, field.rs:340-375); ctx: api.RescueContext ----
def rescue_permutation_dev(ctx, states, out=None):
    """rescue_permutation per state: states (n, 4, L) int64 CUDA tensor, Montgomery form; out may be states itself (in place)."""
    _check(states, shape=(None, ctx.width, _FIELD_LIMBS[ctx.field]))
    out = _out_tensor(out, states.shape, states.device)
    _lib.check(_lib.load().plk_rescue_permutation_dev(states.shape[0], ctx.handle, _dp(states), _dp(out), _stream()))
    return out


def rescue_sponge_dev(ctx, inputs, num_outputs, out=None):
    """rescue_sponge per row: inputs (n, n_inputs, L) int64 CUDA tensor (n_inputs may be 0) -> (n, num_outputs, L).  One launch."""
    L = _FIELD_LIMBS[ctx.field]
    _check(inputs, shape=(None, None, L))
    n, n_inputs = inputs.shape[0], inputs.shape[1]
    out = _out_tensor(out, (n, num_outputs, L), inputs.device)
    _lib.check(_lib.load().plk_rescue_sponge_dev(n, ctx.handle, n_inputs, _dp(inputs), num_outputs, _dp(out), _stream()))
    return out


def rescue_hash_to_curve_dev(ctx, curve, count, seed_start=0, out=None, device="cuda"):
    """hash_usize_to_curve (hash_to_curve.rs:8-11, 78-104) of the integers seed_start .. seed_start + count - 1 on the device; ctx: an
    api.RescueContext over the curve's base field, its rounds standing for security_bits.  (count, 2, L) int64 tensor that
    msm_precompute_dev takes as it is."""
    out = _out_tensor(out, (count, 2, _CURVE_LIMBS[curve]), device)
    assert out.is_cuda  # a fresh one too: `device` is the caller's word
    _call(_lib.load().plk_rescue_hash_to_curve_dev(count, ctx.handle, curve, int(seed_start), _dp(out), _stream()), refusal=True)
    return out


def rescue_hash_field_to_curve_dev(ctx, curve, seeds, out=None):
    """hash_base_field_to_curve per row: seeds (count, L) int64 CUDA tensor, Montgomery form -> (count, 2, L)."""
    L = _CURVE_LIMBS[curve]
    _check(seeds, shape=(None, L))
    count = seeds.shape[0]
    out = _out_tensor(out, (count, 2, L), seeds.device)
    _call(_lib.load().plk_rescue_hash_field_to_curve_dev(count, ctx.handle, curve, _dp(seeds), _dp(out), _stream()), refusal=True)
    return out


def kth_root_dev(field, x, k, out=None):
    """Field::kth_root_u32(k) per element: x (n, L) int64 CUDA tensor; out may be x itself."""
    _check(x, last=(_FIELD_LIMBS[field],))
    out = _out_tensor(out, x.shape, x.device)
    _lib.check(_lib.load().plk_field_kth_root_dev(x.numel() // x.shape[-1], field, int(k), _dp(x), _dp(out), _stream()))
    return out


# ---- gate witness rows on device-resident tables (include/plonky_hip_trace.h, gate_trace.hip) ----
def _trace_tables_dev(n_rows, count, first_rows, wires, constants, status, device):
    _check(first_rows, torch.int32, numel=count)
    wires = torch.zeros((9, n_rows, 4), dtype=torch.int64, device=device) if wires is None else _out_tensor(wires, (9, n_rows, 4), device)
    if constants is not None:
        _check(constants, shape=(6, n_rows, 4))
    return (wires,) + _status(status, 4, device)


def trace_rescue_permutation_dev(ctx, inputs, n_rows, first_rows, wires=None, constants=None, status=None):
    """The blocks of the in-circuit Rescue permutation written into a device-resident wire table: inputs (count, 4, 4) int64 CUDA
    tensor, first_rows (count,) int32, wires (9, n_rows, 4) the prover's table, written in place (None: a fresh table of zeros),
    constants (optional) the (6, n_rows, 4) n-point columns, whose block rows are then written too.  Asynchronous on the current
    stream.  Returns wires; with status=True (or a (4,) int32 CUDA tensor) also the status words: [0] blocks that would pass n_rows
    (nothing of them is written), [1] 0, [2] -1, [3] 0."""
    _check(inputs, shape=(None, ctx.width, 4))
    count = inputs.shape[0]
    wires, status, sp = _trace_tables_dev(n_rows, count, first_rows, wires, constants, status, inputs.device)
    _call(_lib.load().plk_trace_rescue_permutation_dev(count, ctx.handle, _dp(inputs), n_rows, _dp(wires), _dp(first_rows), _dp(constants), sp, _stream()),
          refusal=True)
    return wires if status is None else (wires, status)


def trace_curve_msm_dev(curve, points, scalars, start, n_bits, n_rows, first_rows, wires=None, constants=None, status=None):
    """The blocks of curve_msm written into a device-resident wire table: points (count, parts, 2, 4) and scalars (count, parts, 4)
    int64 CUDA tensors (the INNER curve's affine points, elements of its base field), start (2, 4) host limbs, n_bits the bits of
    the chain; tables as trace_rescue_permutation_dev.  Status words: [0] blocks that would pass n_rows, [1] instances that met an
    exceptional case (their rows from that one on are zero), [2] the first (-1: none).  Such an instance is a result, not an error."""
    _check(points, shape=(None, None, 2, 4))
    count, parts = points.shape[:2]
    _check(scalars, shape=(count, parts, 4))
    wires, status, sp = _trace_tables_dev(n_rows, count, first_rows, wires, constants, status, points.device)
    _call(_lib.load().plk_trace_curve_msm_dev(count, parts, int(n_bits), curve, _dp(points), _dp(scalars), _hp(_u64(start, 2, 4)), n_rows, _dp(wires),
                                              _dp(first_rows), _dp(constants), sp, _stream()), refusal=True)
    return wires if status is None else (wires, status)


# ---- a point times a scalar of its own and the Halo endomorphism on device-resident tensors (scalar_mul.hip) ----
def _scalar_mul_tensors(curve, scalars, points, zero, out, out_zero):
    L = _CURVE_LIMBS[curve]
    _check(scalars, last=(4,))
    _check(points, last=(2, L))
    ns, npts = scalars.numel() // 4, points.numel() // (2 * L)
    count = max(ns, npts)
    if zero is not None:
        _check(zero, torch.uint8, numel=npts)
    out = _out_tensor(out, (count, 2, L), points.device, check="numel")
    out_zero = _out_tensor(out_zero, (count,), points.device, torch.uint8, check="numel")
    return count, ns, npts, _dp(scalars), _dp(points), _dp(zero), _dp(out), _dp(out_zero), out, out_zero


def scalar_mul_dev(curve, scalars, points, zero=None, out=None, out_zero=None):
    """out_i = [s_i] P_i: scalars (n, 4) or (1, 4), points (n, 2, L) or (1, 2, L) int64 CUDA tensors (Montgomery), zero: uint8 flags of
    the points or None.  out may be `points` itself when there are n points.  Returns (out, out_zero)."""
    count, ns, npts, s, p, z, o, oz, out, out_zero = _scalar_mul_tensors(curve, scalars, points, zero, out, out_zero)
    _lib.check(_lib.load().plk_curve_scalar_mul_dev(count, curve, ns, s, npts, p, z, o, oz, _stream()))
    return out, out_zero


def halo_n_dev(curve, scalars, security_bits=128, out=None):
    """n(s_i) of the low security_bits bits: scalars (n, 4) int64 CUDA tensor; out may be scalars itself."""
    _check(scalars, last=(4,))
    out = _out_tensor(out, scalars.shape, scalars.device)
    _lib.check(_lib.load().plk_halo_n_dev(scalars.numel() // 4, curve, int(security_bits), _dp(scalars), _dp(out), _stream()))
    return out


def halo_n_mul_dev(curve, scalars, points, zero=None, security_bits=128, out=None, out_zero=None):
    """out_i = [n(s_i)] P_i by Algorithm 1; tensors as scalar_mul_dev."""
    count, ns, npts, s, p, z, o, oz, out, out_zero = _scalar_mul_tensors(curve, scalars, points, zero, out, out_zero)
    _lib.check(_lib.load().plk_halo_n_mul_dev(count, curve, int(security_bits), ns, s, npts, p, z, o, oz, _stream()))
    return out, out_zero
