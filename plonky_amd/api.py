"""Host-side mirror of the reference's hot-path interface, same names and argument meaning.

  reference (Rust, generic over F / C)                        here
  ------------------------------------------------------------------------------------------
  fft_precompute::<F>(degree)              fft.rs:47      fft_precompute(field, degree)
  fft_with_precomputation(c, &pre)         fft.rs:61      fft_with_precomputation(c, pre)
  fft_with_precomputation_power_of_2       fft.rs:103     fft_with_precomputation_power_of_2(c, pre)
  ifft_with_precomputation_power_of_2      fft.rs:82      ifft_with_precomputation_power_of_2(p, pre)
  fft(c)                                   fft.rs:42      fft(field, c)
  msm_precompute::<C>(generators, w)       curve_msm.rs:27   msm_precompute(curve, generators, w)
  msm_execute(&pre, scalars)               curve_msm.rs:63   msm_execute(pre, scalars)
  msm_execute_parallel(&pre, scalars)      curve_msm.rs:102  msm_execute_parallel(pre, scalars)
  msm_parallel(scalars, generators, w)     curve_msm.rs:54   msm_parallel(curve, scalars, generators, w)

The generic type parameter becomes an explicit field / curve id.  Field elements are numpy
uint64 arrays of shape (n, 4) -- exactly the reference's `limbs` arrays (Montgomery form);
generators are (n, 2, L) arrays (x, y) plus an optional zero-flag vector.  MSM results are the
affine point `(xy, zero)` = ProjectivePoint::to_affine() of the reference's return value.

Error behaviour follows the reference: contract violations raise (the reference panics):
length mismatch (curve_msm.rs:67,106) -> AssertionError; non power of two (util.rs:17) ->
AssertionError; beyond the 2-adicity (field.rs:430) -> AssertionError.

Every function calls the HIP library through the C ABI; there is no CPU implementation here.
"""
import ctypes

import numpy as np

from . import lib as _lib

TWEEDLEDEE_BASE, TWEEDLEDUM_BASE, BLS12_377_SCALAR, BLS12_377_BASE, PALLAS_BASE, VESTA_BASE = 0, 1, 2, 3, 4, 5
TWEEDLEDEE, TWEEDLEDUM, BLS12_377, PALLAS, VESTA = 0, 1, 2, 3, 4

_FIELD_LIMBS = {0: 4, 1: 4, 2: 4, 3: 6, 4: 4, 5: 4}
_CURVE_LIMBS = {0: 4, 1: 4, 2: 6, 3: 4, 4: 4}
_TWO_ADICITY = {0: 34, 1: 33, 2: 47, 3: 46, 4: 32, 5: 32}
CURVE_SCALAR_FIELD = {0: 1, 1: 0, 2: 2, 3: 5, 4: 4}
CURVE_BASE_FIELD = {0: 0, 1: 1, 2: 3, 3: 4, 4: 5}


def log2_ceil(n):  # util.rs:2-9
    r = 0
    while (1 << r) < n:
        r += 1
    return r


def log2_strict(n):  # util.rs:12-19 (panics when n is not a power of two)
    r = log2_ceil(n)
    assert n == 1 << r, "Not a power of two"
    return r


# ---- the marshalling and error layer: every wrapper below is its shapes, its outputs and one _call ----
def _u64(x, *shape):
    """host limbs as a contiguous uint64 array, of that shape when one is given"""
    a = np.ascontiguousarray(x, dtype=np.uint64)
    return a.reshape(*shape) if shape else a


def _as(dtype, x, *shape):
    """_u64 for the other dtypes (flags and bytes, wire ids); None stays None"""
    if x is None:
        return None
    a = np.ascontiguousarray(x, dtype=dtype)
    return a.reshape(*shape) if shape else a


def _u8(x, *shape):
    return _as(np.uint8, x, *shape)


# Limb counts.  An id outside the tables is a KeyError in Python, EXCEPT in the four wrappers that ask with strict=False (rescue_mds,
# RescueContext, hash_usize_to_curve, kth_root): those shape their arrays with 4 limbs and leave the refusal to the library.  The
# wrappers that never look a count up (4-limb scalars, entries that exist for the 4-limb fields only) send a bad id on as well.
def _field_limbs(field, strict=True):
    return _FIELD_LIMBS[field] if strict else _FIELD_LIMBS.get(field, 4)


def _curve_limbs(curve, strict=True):
    return _CURVE_LIMBS[curve] if strict else _CURVE_LIMBS.get(curve, 4)


def _elems(field, a):
    return _u64(a, -1, _FIELD_LIMBS[field])


def _points(curve, generators):
    return _u64(generators, -1, 2, _CURVE_LIMBS[curve])


def _scalar(x):
    """one scalar: 4 limbs whatever the curve"""
    return _u64(x, 4)


def _scalars(x):
    return _u64(x, -1, 4)


def _ptr(a):
    """the host pointer of an array; None for None"""
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _ptrs(arrays, null_empty=False):
    """a ctypes array of the host pointers of these arrays (or of one array's rows); null_empty: an array with nothing in it is a
    null entry, and the array itself never has length 0"""
    if null_empty:
        return (ctypes.c_void_p * max(1, len(arrays)))(*[a.ctypes.data if a.size else None for a in arrays])
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


_NO_INVERSE = ("No inverse", "No inverse")  # field.rs:266 and the Div of field.rs: the reference's panic, as _call takes it


def _call(rc, panics=(), message=None, refusal=False):
    """The one status check.  A PLK_ERR_INVALID_ARG whose text starts with one of `panics` is a panic of the reference: AssertionError
    (explicit, so it survives python -O) with `message`, or with the library's text when there is none.  refusal: any other
    PLK_ERR_INVALID_ARG is ValueError(text).  Everything else is lib.check's PlonkyHipError."""
    if rc == _lib.PLK_OK:
        return
    if rc == _lib.PLK_ERR_INVALID_ARG and (panics or refusal):
        text = _lib.load().plk_last_error().decode("utf-8", "replace")
        if panics and text.startswith(panics):
            raise AssertionError(text if message is None else message)
        if refusal:
            raise ValueError(text)
    _lib.check(rc)


def init_devices(n_devices=0):
    """Run the host-pointer entry points over several GPUs from this one process (plk_init_devices): 0 = PLK_NGPU or every
    visible device; with PLK_VIRTUAL_DEVICES=k, k logical devices on one physical GPU.  Returns the number of logical devices."""
    L = _lib.load()
    _call(L.plk_init_devices(int(n_devices)))
    return int(L.plk_device_count())


def device_count():
    return int(_lib.load().plk_device_count())


class FftPrecomputation:
    """fft.rs:28-40.  The reference stores host tables (subgroups_rev); the device tables live
    in the library's cache keyed by (device, field, log n), so this object only records the
    size -- it stays plain data, as the reference's serde-able struct is."""

    def __init__(self, field, degree_pow):
        self.field = field
        self.degree_pow = degree_pow

    def size(self):
        return 1 << self.degree_pow


def fft_precompute(field, degree):
    degree_pow = log2_ceil(degree)
    assert degree_pow <= _TWO_ADICITY[field], "n_power <= TWO_ADICITY"  # field.rs:430
    _call(_lib.load().plk_ntt_precompute(field, degree_pow))
    return FftPrecomputation(field, degree_pow)


def fft_precompute_table(field, degree):
    """The CONTENTS of the reference's FftPrecomputation (fft.rs:28-59), built on the device: the list subgroups_rev[i],
    i = 0 ..= log2_ceil(degree), each a (2^i, L) array of the bit-reversed powers of primitive_root_of_unity(i) (L = 4 limbs; 6 for
    Bls12377Base)."""
    degree_pow = log2_ceil(degree)
    assert degree_pow <= _TWO_ADICITY[field], "n_power <= TWO_ADICITY"  # field.rs:430
    flat = np.empty(((2 << degree_pow) - 1, _field_limbs(field)), dtype=np.uint64)
    _call(_lib.load().plk_ntt_precompute_table(field, degree_pow, _ptr(flat)))
    return [flat[(1 << i) - 1: (2 << i) - 1] for i in range(degree_pow + 1)]


def _ntt(field, log_n, inverse, x):
    out = np.empty_like(x)
    _call(_lib.load().plk_ntt(field, log_n, 1 if inverse else 0, _ptr(x), _ptr(out)))
    return out


def fft_with_precomputation_power_of_2(coefficients, precomputation):
    x = _elems(precomputation.field, coefficients)
    degree_pow = log2_strict(x.shape[0])
    # fft.rs:107-111 debug_assert_eq!: release builds accept any table at least as large (Appendix A.7)
    assert degree_pow <= _TWO_ADICITY[precomputation.field]
    return _ntt(precomputation.field, degree_pow, False, x)


def ifft_with_precomputation_power_of_2(points, precomputation):
    x = _elems(precomputation.field, points)
    degree_pow = log2_strict(x.shape[0])
    assert degree_pow <= _TWO_ADICITY[precomputation.field]
    return _ntt(precomputation.field, degree_pow, True, x)


def fft_with_precomputation(coefficients, precomputation):
    x = _elems(precomputation.field, coefficients)
    degree = x.shape[0]
    log_n = log2_ceil(degree)
    if degree == 1 << log_n:
        return fft_with_precomputation_power_of_2(x, precomputation)
    out = np.empty((1 << log_n, x.shape[1]), dtype=np.uint64)
    _call(_lib.load().plk_ntt_padded(precomputation.field, log_n, _ptr(x), degree, _ptr(out)))
    return out


def fft(field, coefficients):
    x = _elems(field, coefficients)
    return fft_with_precomputation(x, fft_precompute(field, x.shape[0]))


def fft_batch(field, polys, inverse=False):
    """`batch` independent power-of-two transforms in one call (the par_iter over the 9 wire
    polynomials, plonk_util.rs:169-190).  polys: (batch, n, 4)."""
    polys = _u64(polys)
    batch, n = polys.shape[0], polys.shape[1]
    log_n = log2_strict(n)
    out = np.empty_like(polys)
    _call(_lib.load().plk_ntt_batch(field, log_n, 1 if inverse else 0, batch, _ptrs(polys), _ptrs(out)))
    return out


# ---- polynomial callers of the NTT (src/polynomial.rs, src/plonk_util.rs) ----
def _pow2_ceil(n):
    return 1 << log2_ceil(max(n, 1))


def polynomial_divide_by_z_h(field, coeffs, n):
    """Polynomial::divide_by_z_h (polynomial.rs:330-380): coeffs / (X^n - 1).  Returns the
    2^ceil(log2(degree + 1)) untrimmed coefficients the reference returns; the zero polynomial
    comes back unchanged."""
    x = _elems(field, coeffs)
    assert n >= 1
    cap = max(x.shape[0], _pow2_ceil(x.shape[0]))
    out = np.zeros((cap, x.shape[1]), dtype=np.uint64)
    out_len = ctypes.c_size_t(0)
    _call(_lib.load().plk_poly_divide_by_z_h(field, _ptr(x), x.shape[0], n, _ptr(out), cap, ctypes.byref(out_len)))
    return out[: out_len.value].copy()


def polynomial_mul(field, a, b):
    """Polynomial::mul (polynomial.rs:208-226)."""
    x, y = _elems(field, a), _elems(field, b)
    cap = _pow2_ceil(x.shape[0] + y.shape[0])
    out = np.zeros((cap, x.shape[1]), dtype=np.uint64)
    out_len = ctypes.c_size_t(0)
    _call(_lib.load().plk_poly_mul(field, _ptr(x), x.shape[0], _ptr(y), y.shape[0], _ptr(out), cap, ctypes.byref(out_len)))
    return out[: out_len.value].copy()


POLY_DIV_MAX_DEGREE = 32  # PLK_POLY_DIV_MAX_DEGREE


def _degree_plus_one(x):
    """Polynomial::degree_plus_one (polynomial.rs:107-112): 0 for the zero polynomial"""
    nz = np.nonzero(x.any(axis=1))[0]
    return int(nz[-1]) + 1 if nz.size else 0


def _division_buffers(x, y, da, db):
    """the trimmed operands and the quotient and remainder buffers of a division with deg a >= deg b >= 1"""
    return _u64(x[:da]), _u64(y[:db]), np.empty((da - db + 1, 4), dtype=np.uint64), np.empty((db - 1, 4), dtype=np.uint64)


def polynomial_division(field, a, b):
    """Polynomial::polynomial_division (polynomial.rs:299-327) -> (q, r) with the reference's lengths in every branch: a zero a gives
    ([0], empty), deg a < deg b gives ([0], a), deg b = 0 gives a / b[0] untrimmed and an empty remainder, otherwise q and r trimmed.
    A zero b raises (the reference panics); a divisor of degree above 32 raises ValueError: the device divides by the linear recurrence
    that a LOW-degree divisor gives (plk_poly_division), the divisor of the public-input quotient (plonk.rs:199-235)."""
    x, y = _elems(field, a), _elems(field, b)
    da, db = _degree_plus_one(x), _degree_plus_one(y)
    empty = np.zeros((0, 4), dtype=np.uint64)
    if db == 0:
        raise ZeroDivisionError("Division by zero polynomial")
    if da == 0:
        return np.zeros((1, 4), dtype=np.uint64), empty
    if da < db:
        return np.zeros((1, 4), dtype=np.uint64), x.copy()
    if db == 1:
        inv = field_op(field, "inverse", y[:1])
        return field_op(field, "mul", x, np.repeat(inv, x.shape[0], axis=0)), empty
    if db - 1 > POLY_DIV_MAX_DEGREE:
        raise ValueError("divisor of degree %d: at most %d (PLK_POLY_DIV_MAX_DEGREE)" % (db - 1, POLY_DIV_MAX_DEGREE))
    xs, ys, q, r = _division_buffers(x, y, da, db)
    _call(_lib.load().plk_poly_division(field, _ptr(xs), da, _ptr(ys), db, _ptr(q), q.shape[0], _ptr(r)))
    return q, r[: _degree_plus_one(r)].copy()


def polynomial_inv_mod_xn(field, h, n):
    """Polynomial::inv_mod_xn (polynomial.rs:261-294): g with g h = 1 mod X^n -> (n, 4); h[0] == 0 raises as the reference panics."""
    x = _elems(field, h)
    assert n >= 1 and x.shape[0] >= 1
    if not x[0].any():
        raise ValueError("Inverse doesn't exist.")
    out = np.empty((n, 4), dtype=np.uint64)
    _call(_lib.load().plk_poly_inv_mod_xn(n, field, _ptr(x), x.shape[0], _ptr(out)))
    return out


def polynomial_div_rem(field, a, b):
    """Polynomial::polynomial_division (polynomial.rs:299-327) -> (q, r) for a divisor of ANY degree (plk_poly_div_rem: the recurrence of
    polynomial_division up to degree 32, the reference's Newton route above), with the reference's lengths in every branch, the branches
    of polynomial_division: a zero a gives ([0], empty), deg a < deg b gives ([0], a), deg b = 0 gives a / b[0] untrimmed and an empty
    remainder, otherwise q and r trimmed.  A zero b raises ZeroDivisionError (the reference panics)."""
    x, y = _elems(field, a), _elems(field, b)
    da, db = _degree_plus_one(x), _degree_plus_one(y)
    if db == 0 or da < db or db == 1:
        return polynomial_division(field, x, y)  # no divisor degree is involved in these branches
    xs, ys, q, r = _division_buffers(x, y, da, db)
    _call(_lib.load().plk_poly_div_rem(da, field, _ptr(xs), _ptr(ys), db, _ptr(q), q.shape[0], _ptr(r)))
    return q, r[: _degree_plus_one(r)].copy()


def polynomial_long_division(field, a, b):
    """Polynomial::polynomial_long_division (polynomial.rs:232-259): the same quotient and remainder; its deg b = 0 case goes through
    the loop and leaves the quotient at deg a + 1 coefficients."""
    x, y = _elems(field, a), _elems(field, b)
    if _degree_plus_one(y) == 1 and _degree_plus_one(x) >= 1:
        return polynomial_division(field, x[: _degree_plus_one(x)], y)
    return polynomial_division(field, a, b)


def polynomial_from_roots(field, roots):
    """prod_i (X - roots[i]) (the fold of plonk.rs:207-215) -> (k + 1, 4), monic; at most 32 roots."""
    r = _scalars(roots)
    out = np.empty((r.shape[0] + 1, 4), dtype=np.uint64)
    _call(_lib.load().plk_poly_from_roots(field, r.shape[0], _ptr(r), _ptr(out)))
    return out


def scale_polynomials(field, polys, alpha, degree):
    """scale_polynomials (plonk_util.rs:283-298): sum_j alpha^j polys[j], the first `degree` coefficients: powers + reduce_polynomials."""
    polys = [_scalars(p) for p in polys]
    assert all(p.shape[0] >= degree for p in polys), "the reference indexes every polynomial up to degree"
    return reduce_polynomials(field, [p[:degree] for p in polys], powers(field, alpha, len(polys)), degree)


def polynomials_to_values_padded(polys, precomputation):
    """plonk_util.rs:179-190: every polynomial padded to 8x its length, then evaluated on the
    precomputation's domain (eval_domain pads further when the domain is larger).  polys: sequence of
    (len_b, 4) arrays; returns (batch, domain, 4)."""
    field = precomputation.field
    ps = [_elems(field, p) for p in polys]
    n = precomputation.size()
    for p in ps:
        assert p.shape[0] * 8 <= n, "fft.rs:107-111: the table is too small for the padded polynomial"
    batch = len(ps)
    out = np.empty((batch, n, 4), dtype=np.uint64)
    if batch == 0:
        return out
    lens = (ctypes.c_size_t * batch)(*[p.shape[0] for p in ps])
    _call(_lib.load().plk_ntt_padded_batch(field, precomputation.degree_pow, batch, _ptrs(ps), lens, _ptrs(out)))
    return out


def values_to_polynomials(values_vec, precomputation):
    """plonk_util.rs:169-177: Polynomial::from_evaluations over a batch."""
    return fft_batch(precomputation.field, values_vec, inverse=True)


class MsmPrecomputation:
    """curve_msm.rs:16-25.  Owns a device context holding the generators and the window tables
    [2^(c j)] G_i.  `w` is kept because it is part of the reference struct; the device window c
    is a tuning choice (the result does not depend on it)."""

    def __init__(self, curve, ctx, n, w):
        self.curve = curve
        self._ctx = ctx
        self.n = n
        self.w = w

    @property
    def window(self):
        return int(_lib.load().plk_msm_ctx_window(self._ctx))

    def __len__(self):
        return self.n

    def free(self):
        if self._ctx:
            _lib.load().plk_msm_free(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


MSM_TABLE_FREE = 1  # PLK_MSM_TABLE_FREE


def msm_precompute(curve, generators, w, zero=None, device_window=0, table_free=False):
    """generators: (n, 2, L) affine x,y Montgomery limbs; zero: optional n flags (AffinePoint.zero).
    The reference takes ProjectivePoints and only ever passes normalised generators
    (circuit_builder.rs:1127-1133); the shim in INTEGRATION.md reads powers_per_generator[i][0].
    table_free: no window tables on the device (generators used once: msm_parallel, the IPA rounds)."""
    g = _points(curve, generators)
    n = g.shape[0]
    z = _u8(zero)
    assert z is None or z.shape[0] == n
    ctx = ctypes.c_void_p()
    _call(_lib.load().plk_msm_precompute_ex(curve, n, _ptr(g), _ptr(z), device_window, MSM_TABLE_FREE if table_free else 0, ctypes.byref(ctx)))
    return MsmPrecomputation(curve, ctx, n, w)


def _msm_execute(entry, rows, precomputation, scalars):
    s = _scalars(scalars)
    # assert_eq!(precomputation.powers_per_generator.len(), scalars.len())  curve_msm.rs:106
    assert s.shape[0] == precomputation.n, "powers_per_generator.len() != scalars.len()"
    out = np.zeros((rows, _curve_limbs(precomputation.curve)), dtype=np.uint64)
    oz = np.zeros(1, dtype=np.uint8)
    _call(getattr(_lib.load(), entry)(precomputation._ctx, _ptr(s), s.shape[0], _ptr(out), _ptr(oz)))
    return out, int(oz[0])


def msm_execute_parallel(precomputation, scalars):
    return _msm_execute("plk_msm_execute", 2, precomputation, scalars)


# msm_execute (serial, curve_msm.rs:63) computes the same group element as msm_execute_parallel.
msm_execute = msm_execute_parallel


def msm_execute_parallel_projective(precomputation, scalars):
    """msm_execute_parallel with its OWN return type (curve_msm.rs:102-157 returns the ProjectivePoint `y`, not normalised):
    ((3, L) x | y | z Montgomery limbs, zero flag).  ProjectivePoint::to_affine / batch_to_affine (curve.rs:206-232) gives the unique point."""
    return _msm_execute("plk_msm_execute_projective", 3, precomputation, scalars)


def msm_execute_batch(precomputation, scalar_vectors):
    """commit_polynomials (plonk_util.rs:215-231): several scalar vectors, same generators."""
    sv = _u64(scalar_vectors)
    batch = sv.shape[0]
    sv = sv.reshape(batch, -1, 4)
    assert sv.shape[1] == precomputation.n, "powers_per_generator.len() != scalars.len()"
    out = np.zeros((batch, 2, _curve_limbs(precomputation.curve)), dtype=np.uint64)
    oz = np.zeros(batch, dtype=np.uint8)
    _call(_lib.load().plk_msm_execute_batch(precomputation._ctx, batch, _ptrs(sv), sv.shape[1], _ptr(out), _ptr(oz)))
    return out, oz


def commitment_precompute(curve, generators, blinding_point, w, device_window=0):
    """Device context for PolynomialCommitment::coeffs_vec_to_commitments (poly_commit.rs:31-66): the blinding term
    [r] H is the (n+1)-th term of the same MSM, so the context simply holds H after the n generators."""
    g = _points(curve, generators)
    h = _points(curve, blinding_point)
    assert h.shape[0] == 1
    return msm_precompute(curve, np.concatenate([g, h]), w, device_window=device_window)


def coeffs_vec_to_commitments(precomputation, coefficients_vec, blinding_factors):
    """poly_commit.rs:51-66: one commitment per coefficient vector, pedersen_hash(coeffs) + [r] H, already normalised
    (the reference's batch_to_affine).  blinding_factors: one Montgomery scalar per vector (zeros when blinding is off).
    precomputation: from commitment_precompute.  Returns (points (k, 2, L), zero flags (k,))."""
    cv = _u64(coefficients_vec)
    k = cv.shape[0]
    cv = cv.reshape(k, -1, 4)
    r = _u64(blinding_factors, k, 1, 4)
    assert cv.shape[1] + 1 == precomputation.n, "coefficients.len() must equal the number of generators (curve_msm.rs:106)"
    return msm_execute_batch(precomputation, np.concatenate([cv, r], axis=1))


def msm_parallel(curve, scalars, generators, w, zero=None):
    """curve_msm.rs:54-61: precompute + execute for generators that are used once -> no device tables."""
    pre = msm_precompute(curve, generators, w, zero=zero, table_free=True)
    try:
        return msm_execute_parallel(pre, scalars)
    finally:
        pre.free()


def msm_precompute_table(curve, generators, w, zero=None):
    """The CONTENTS of the reference's MsmPrecomputation (curve_msm.rs:16-52): powers_per_generator[i][j] = [2^(w j)] G_i,
    j < ceil(ScalarField::BITS / w).  Returns (table (n, digits, 2, L), zero flags (n, digits))."""
    g = _points(curve, generators)
    n, L = g.shape[0], g.shape[2]
    digits = int(_lib.load().plk_msm_table_digits(curve, w))
    assert digits > 0
    z = _u8(zero)
    out = np.zeros((n, digits, 2, L), dtype=np.uint64)
    oz = np.zeros((n, digits), dtype=np.uint8)
    _call(_lib.load().plk_msm_precompute_table(curve, n, _ptr(g), _ptr(z), w, _ptr(out), _ptr(oz)))
    return out, oz


def fold_generators(curve, g_lo, g_hi, scalar_lo, scalar_hi, lo_zero=None, hi_zero=None):
    """The generator fold of an IPA round (halo.rs:119-123): out_i = [scalar_lo] g_lo_i + [scalar_hi] g_hi_i, where the
    reference calls msm_parallel(&[u_inv, u], &[g_lo_i, g_hi_i], 4) per pair.  Points (m, 2, L) affine Montgomery
    limbs, scalars (4,) Montgomery limbs in the curve's scalar field.  Returns (out (m, 2, L), zero flags (m,))."""
    lo, hi = _points(curve, g_lo), _points(curve, g_hi)
    m = lo.shape[0]
    assert hi.shape[0] == m
    a, b = _scalar(scalar_lo), _scalar(scalar_hi)
    lz, hz = _u8(lo_zero), _u8(hi_zero)
    out = np.zeros_like(lo)
    oz = np.zeros(m, dtype=np.uint8)
    _call(_lib.load().plk_curve_fold_pairs(curve, m, _ptr(lo), _ptr(lz), _ptr(hi), _ptr(hz), _ptr(a), _ptr(b), _ptr(out), _ptr(oz)))
    return out, oz


def curve_sum_affine(curve, points, zero=None):
    """Adds k affine points (per-GPU partial MSM results after the all-gather)."""
    p = _points(curve, points)
    z = _u8(zero)
    out = np.zeros((2, p.shape[2]), dtype=np.uint64)
    oz = np.zeros(1, dtype=np.uint8)
    _call(_lib.load().plk_curve_sum_affine(curve, p.shape[0], _ptr(p), _ptr(z), _ptr(out), _ptr(oz)))
    return out, int(oz[0])


def affine_summation_best(curve, summation, zero=None):
    """curve_summations.rs:18-22 (and the _pairwise / _batch_inversion forms it chooses between, :39-58 / :60-68: one group element,
    whatever the form): the sum of a list of affine points, identity operands, P = Q and P = -Q included.  On the device the list is
    one workgroup's XYZZ sum (k_sum_affine); returns ((2, L) affine limbs, zero flag)."""
    return curve_sum_affine(curve, summation, zero)


def affine_multisummation_best(curve, summations, zeros=None):
    """curve_summations.rs:24-35: k independent sums of affine points -> k points, one device sum per list (inside the MSM the
    reference's call site, curve_msm.rs:131-145, is replaced by the bucket accumulation - DESIGN.md section 5)."""
    _curve_limbs(curve)  # a bad id is refused here, with no list as well
    return [curve_sum_affine(curve, pts, None if zeros is None else zeros[k]) for k, pts in enumerate(summations)]


FIELD_OPS = {"add": 0, "sub": 1, "mul": 2, "neg": 3, "square": 4, "inverse": 5, "to_canonical": 6, "from_canonical": 7,
             "inverse_euclid": 8, "inverse_divsteps": 9, "inverse_divsteps_var": 10, "inverse_divsteps_one_lane": 11,
             "mul_add2_edge": 12, "wide_sum": 13, "sqrt": 14, "sqrt_tabled": 15}
FIELD_OP_NO_ROOT = 0xFFFFFFFFFFFFFFFF  # every limb of what "sqrt" / "sqrt_tabled" write for a non-residue: no reduced element of any field


def field_op(field, op, a, b=None):
    """Element-wise device field arithmetic (parity tests of the HIP field code).  "sqrt" is Field::square_root by the reference's
    squarings (fe_sqrt), "sqrt_tabled" the same root from the table of powers the hashes to the curve use (fe_sqrt_tabled)."""
    a = _elems(field, a)
    out = np.empty_like(a)
    bb = a if b is None else _elems(field, b)
    _call(_lib.load().plk_field_op(field, FIELD_OPS[op], _ptr(a), _ptr(bb), _ptr(out), a.shape[0]))
    return out


CURVE_OPS = {"add": 0, "dbl": 1, "add_q": 2, "dbl_q": 3, "madd": 4, "madd_entry": 5, "dbl_q_times": 6, "wave_sum_q": 7, "chain_q": 8}
CURVE_OP_INFLATE, CURVE_OP_NEGATE = 1, 2


def curve_op(curve, op, a, b=None, flags=None, param=0):
    """Element-wise device point arithmetic (plk_curve_op: parity tests of ecz.cuh / ecz_coop.cuh).  a, b: (points (n, 2, L), identity
    flags (n,) or None, lambdas (n, L)).  Returns (affine results (m, 2, L), zero flags (m,), mismatch word); m = ceil(n / param) for
    "wave_sum_q", n otherwise."""
    L = _curve_limbs(curve)
    axy, az, al = _u64(a[0], -1, 2, L), _u8(a[1]), _u64(a[2], -1, L)
    n = axy.shape[0]
    bxy, bz, bl = (None, None, None) if b is None else (_u64(b[0], n, 2, L), _u8(b[1]), None if b[2] is None else _u64(b[2], n, L))
    fl = np.zeros(n, dtype=np.uint8) if flags is None else _u8(flags)
    code = CURVE_OPS[op]
    m = -(-n // param) if code == 7 else n
    out, oz, mism = np.zeros((m, 2, L), dtype=np.uint64), np.zeros(m, dtype=np.uint8), ctypes.c_uint(0xFFFFFFFF)
    _call(_lib.load().plk_curve_op(curve, code, param, n, _ptr(axy), _ptr(az), _ptr(al), _ptr(bxy), _ptr(bz), _ptr(bl), _ptr(fl), _ptr(out), _ptr(oz),
                                   ctypes.byref(mism)))
    return out, oz, int(mism.value)


def msm_debug_digits(curve, scalars, window_bits):
    """The MSM's digit recoding on its own (to_digits, curve_msm.rs:159-180): scalars (n, 4) Montgomery limbs in the curve's scalar field
    -> (n, ceil((BITS + 1) / w)) signed digits as the ordering kernels form them, and the reference's unsigned digits rebuilt from them
    (u_j = d_j - carry_j + 2^w carry_(j+1), carry_(j+1) = [d_j - carry_j < 0]), and the carry out of the top window (always 0: it has room)."""
    s = _scalars(scalars)
    nd = ctypes.c_uint()
    _call(_lib.load().plk_msm_debug_digits(curve, window_bits, 0, None, None, ctypes.byref(nd)))
    d = np.zeros((s.shape[0], nd.value), dtype=np.int32)
    _call(_lib.load().plk_msm_debug_digits(curve, window_bits, s.shape[0], _ptr(s), _ptr(d), ctypes.byref(nd)))
    # carry_(j+1) = [d_j - carry_j < 0]: a negative digit borrowed from the next window, and so did a ZERO digit that stands for
    # 2^w - 1 + carry_j = 2^w (the device has no entry for it: magnitude 0, carry out)
    unsigned = np.zeros(d.shape, dtype=np.int64)
    carry = np.zeros(s.shape[0], dtype=np.int64)
    for j in range(nd.value):
        v = d[:, j].astype(np.int64) - carry
        carry = (v < 0).astype(np.int64)
        unsigned[:, j] = v + (carry << window_bits)
    return d, unsigned, carry


# ---- the Plonk quotient numerator (plonk.rs:375-456, gates/) ----
NUM_WIRES, NUM_ROUTED_WIRES, NUM_CONSTANTS, GRID_WIDTH = 9, 6, 6, 65  # plonk.rs:21-25


def evaluate_all_constraints(field, local_constant_values, local_wire_values, right_wire_values, below_wire_values, inner_zeta, inner_a):
    """gates/mod.rs:46-125 at `count` points: constants (count, 6, 4), wires (count, 9, 4) x 3 -> (count, 8, 4).
    inner_zeta / inner_a: InnerC::ZETA and InnerC::A (4 limbs, Montgomery) - how InnerC enters the curve gates."""
    k = _u64(local_constant_values, -1, NUM_CONSTANTS, 4)
    l, r, b = (_u64(x, -1, NUM_WIRES, 4) for x in (local_wire_values, right_wire_values, below_wire_values))
    count = k.shape[0]
    assert l.shape[0] == r.shape[0] == b.shape[0] == count
    zeta, a = _scalar(inner_zeta), _scalar(inner_a)
    out = np.empty((count, 8, 4), dtype=np.uint64)
    _call(_lib.load().plk_plonk_evaluate_all_constraints(field, count, _ptr(k), _ptr(l), _ptr(r), _ptr(b), _ptr(zeta), _ptr(a), _ptr(out)))
    return out


WITNESS_NONE = 0xFFFFFFFF  # report words [1] and [4] when nothing failed


class WitnessReport:
    """What check_witness returns (include/plonky_hip_witness.h): bad_rows gate rows whose unified constraint set is not all zero,
    first_row the smallest of them (None when there is none), first_mask its mask (bit t: term t is nonzero), first_terms (8, 4)
    its eight terms (what evaluate_all_constraints returns for it; zeros when no row fails); bad_copies routed wires that differ from
    their neighbour under sigma, first_copy the smallest as (input, gate) (None when there is none), sigma_out_of_range entries of
    sigma that are not below 6n (counted, not followed); row_masks (n,) uint8 or None."""

    def __init__(self, degree, report, first_terms=None, row_masks=None):
        words = [int(w) for w in np.asarray(report).reshape(8).view(np.uint32)]
        self.degree = degree
        self.bad_rows = words[0]
        self.first_row = None if words[1] == WITNESS_NONE else words[1]
        self.first_mask = words[2]
        self.bad_copies = words[3]
        self.first_copy = None if words[4] == WITNESS_NONE else (words[4] // degree, words[4] % degree)
        self.sigma_out_of_range = words[5]
        self.first_terms = first_terms
        self.row_masks = row_masks

    @property
    def ok(self):
        return self.bad_rows == 0 and self.bad_copies == 0 and self.sigma_out_of_range == 0

    def message(self):
        """the reference's own words for the first failing gate (plonk.rs:158-167); None when every gate is satisfied"""
        return None if self.first_row is None else "%d-th gate constraints are not satisfied" % self.first_row


def check_witness(field, degree, constants, wires, sigma=None, inner_zeta=None, inner_a=None, constants_stride=1, row_masks=False):
    """The witness check (plk_plonk_check_witness; the debug-build check of plonk.rs:158-167 without its O(n^2)): constants
    (6, degree * constants_stride, 4) - the n-point selector columns, or constants_8n with constants_stride=8 -, wires
    wire_values_by_wire_index (9, degree, 4), sigma (optional) the 6 degree entries of to_sigma; inner_zeta / inner_a as for
    evaluate_all_constraints (both are needed).  Returns a WitnessReport; row_masks=True also brings back the mask of every row.
    A witness that fails is a result: nothing is raised for it."""
    log_degree = log2_strict(degree)
    assert constants_stride in (1, 8), "constants_stride must be 1 or 8"
    assert inner_zeta is not None and inner_a is not None, "inner_zeta and inner_a are needed"
    k = _u64(constants, NUM_CONSTANTS, degree * constants_stride, 4)
    w = _u64(wires, NUM_WIRES, degree, 4)
    sg = _as(np.uint32, sigma, NUM_ROUTED_WIRES * degree)
    zeta, a = _scalar(inner_zeta), _scalar(inner_a)
    report = np.zeros(8, dtype=np.uint32)
    masks = np.zeros(degree, dtype=np.uint8) if row_masks else None
    terms = np.zeros((8, 4), dtype=np.uint64)
    _call(_lib.load().plk_plonk_check_witness(log_degree, field, _ptr(k), constants_stride, _ptr(w), _ptr(sg), _ptr(zeta), _ptr(a), _ptr(report), _ptr(masks),
                                              _ptr(terms)), refusal=True)
    return WitnessReport(degree, report, terms, masks)


def vanishing_points(field, degree, constants_8n, wire_values_8n, s_sigma_values_8n, plonk_z_points_8n, k_is, alpha, beta, gamma, inner_zeta, inner_a):
    """The 8n-point loop of Prover::vanishing_poly (plonk.rs:392-453); Polynomial::from_evaluations of the result
    (ifft_with_precomputation_power_of_2) is the vanishing polynomial.  Tables: (6, 8n, 4), (9, 8n, 4), (6, 8n, 4), (8n, 4)."""
    log_degree = log2_strict(degree)
    n8 = 8 * degree
    c = _u64(constants_8n, NUM_CONSTANTS, n8, 4)
    w = _u64(wire_values_8n, NUM_WIRES, n8, 4)
    s = _u64(s_sigma_values_8n, NUM_ROUTED_WIRES, n8, 4)
    z = _u64(plonk_z_points_8n, n8, 4)
    ks = _u64(k_is, NUM_ROUTED_WIRES, 4)
    sc = [_scalar(x) for x in (alpha, beta, gamma, inner_zeta, inner_a)]
    out = np.empty((n8, 4), dtype=np.uint64)
    _call(_lib.load().plk_plonk_vanishing_points(field, log_degree, _ptr(c), _ptr(w), _ptr(s), _ptr(z), _ptr(ks), *map(_ptr, sc), _ptr(out)))
    return out


def permutation_polynomial(field, degree, wire_values, s_sigma_values, k_is, beta, gamma, sigma_stride=8):
    """permutation_polynomial (plonk_util.rs:234-262): Z on the n-subgroup, (n, 4).  wire_values: wire_values_by_wire_index,
    (>= 6, n, 4) (rows 0..5 are read); s_sigma_values: (6, n * sigma_stride, 4) - s_sigma_values_8n with the default stride 8,
    the n-point sigma values with stride 1.  A zero denominator in rows 0..n-2 panics in the reference ("No inverse") ->
    AssertionError here."""
    log_degree = log2_strict(degree)
    assert sigma_stride in (1, 8), "sigma_stride must be 1 or 8"
    w = np.asarray(wire_values, dtype=np.uint64).reshape(-1, degree, 4)
    assert w.shape[0] >= NUM_ROUTED_WIRES
    w = _u64(w[:NUM_ROUTED_WIRES])  # the first six rows, then contiguous
    s = _u64(s_sigma_values, NUM_ROUTED_WIRES, degree * sigma_stride, 4)
    ks = _u64(k_is, NUM_ROUTED_WIRES, 4)
    b, g = _scalar(beta), _scalar(gamma)
    out = np.empty((degree, 4), dtype=np.uint64)
    # the reference panics (plonk_util.rs:259, field.rs Div)
    _call(_lib.load().plk_plonk_permutation_z(field, log_degree, _ptr(w), _ptr(s), sigma_stride, _ptr(ks), _ptr(b), _ptr(g), _ptr(out), None), *_NO_INVERSE)
    return out


# ---- the copy-constraint partitions and sigma (src/partition.rs, plonk_util.rs:264-280) ----
class TargetPartitions:
    """TargetPartitions (partition.rs:6-82), a host mirror.  Targets are hashable tuples: ("wire", gate, input) for Target::Wire and
    ("virtual", index) for every other target (to_wire_partitions drops them).  The union-find stays on the host: the order of a
    partition's members is the order in which merge appended the lists, and sigma - hence c_s_sigmas - depends on it."""

    def __init__(self):
        self.partitions = []
        self.indices = {}

    def get_partition(self, target):
        return self.partitions[self.indices[target]]

    def add_partition(self, target):  # partition.rs:30-34
        self.indices[target] = len(self.partitions)
        self.partitions.append([target])

    def merge(self, a, b):
        """partition.rs:38-52: a's list is appended to b's and a's members are re-pointed; a's old list stays where it is (the Rust
        clones it), so a merged-away index keeps a stale list that no target points to."""
        a_index, b_index = self.indices[a], self.indices[b]
        if a_index != b_index:
            a_partition = list(self.partitions[a_index])
            for sibling in a_partition:
                self.indices[sibling] = b_index
            self.partitions[b_index].extend(a_partition)

    def to_wire_partitions(self):  # partition.rs:54-81
        partitions = [[(t[1], t[2]) for t in old if t[0] == "wire"] for old in self.partitions]
        indices = {(t[1], t[2]): index for t, index in self.indices.items() if t[0] == "wire"}
        result = WirePartitions(partitions, indices)
        result.assert_valid()
        return result


class WirePartitions:
    """WirePartitions (partition.rs:84-137): wires are (gate, input) pairs."""

    def __init__(self, partitions, indices):
        self.partitions = partitions
        self.indices = indices

    def assert_valid(self):  # partition.rs:90-102
        for partition in self.partitions:
            for _, inp in partition:
                if inp >= NUM_ROUTED_WIRES:
                    assert len(partition) == 1, "Non-routed wires should not be in a partition containing other wires"

    def get_neighbor(self, wire):  # partition.rs:108-118
        partition = self.partitions[self.indices[wire]]
        n = len(partition)
        for i in range(n):
            if partition[i] == wire:
                return partition[(i + 1) % n]
        raise AssertionError("Wire not found in the expected partition")

    def to_sigma(self):
        """partition.rs:122-136, the reference's own loop (a linear scan per wire): for small sizes and tests; the device form is
        to_csr + wire_partitions_to_sigma / device.sigma_dev."""
        assert len(self.indices) % NUM_WIRES == 0
        num_gates = len(self.indices) // NUM_WIRES
        sigma = []
        for inp in range(NUM_ROUTED_WIRES):
            for gate in range(num_gates):
                g, i = self.get_neighbor((gate, inp))
                sigma.append(i * num_gates + g)
        return sigma

    def to_csr(self, degree):
        """The flattened form plk_plonk_sigma[_dev] takes: (members, offsets) uint32 arrays over the LIVE partitions - those some wire's
        index still points to, in the order of their indices; the stale lists merge leaves behind are dropped.  A member is the
        wire id input * degree + gate."""
        live = sorted(set(self.indices.values()))
        offsets = np.zeros(len(live) + 1, dtype=np.uint32)
        members = []
        for k, q in enumerate(live):
            members.extend(inp * degree + gate for gate, inp in self.partitions[q])
            offsets[k + 1] = len(members)
        return np.array(members, dtype=np.uint32), offsets


_SIGMA_PANICS = ("Non-routed wires", "no entry found for key", "wire id out of range")  # the reference's panics behind plk_plonk_sigma


def wire_partitions_to_sigma(field, degree, members, offsets, k_is, want_values=True):
    """to_sigma + sigma_polynomials through the device (plk_plonk_sigma; host arrays, copied through PCIe): members / offsets as
    WirePartitions.to_csr gives them, k_is (6, 4) -> (sigma (6 degree,) uint32, s_sigma (6, degree, 4)).  Where the reference panics
    (a routed wire that is not listed exactly once, a non-routed wire in company) -> AssertionError with the library's text."""
    log_degree = log2_strict(degree)
    m, o = _as(np.uint32, members, -1), _as(np.uint32, offsets, -1)
    assert o.shape[0] >= 1, "offsets holds num_partitions + 1 entries"
    assert int(o[-1]) == m.shape[0], "offsets[num_partitions] must be the number of members"
    ks = _u64(k_is, NUM_ROUTED_WIRES, 4)
    sigma = np.empty(NUM_ROUTED_WIRES * degree, dtype=np.uint32)
    values = np.empty((NUM_ROUTED_WIRES, degree, 4), dtype=np.uint64) if want_values else None
    _call(_lib.load().plk_plonk_sigma(log_degree, field, _ptr(m), _ptr(o), o.shape[0] - 1, _ptr(ks), _ptr(sigma), _ptr(values)), _SIGMA_PANICS)
    return (sigma, values) if want_values else sigma


def sigma_polynomials(field, sigma, degree, k_is):
    """sigma_polynomials (plonk_util.rs:264-280): sigma, 6 degree entries below 6 degree -> (6, degree, 4), element (j, r) =
    k_is[x / degree] g^(x % degree) for x = sigma[j degree + r].  The values of the identity permutation come from the device
    (plk_plonk_sigma over singletons); sigma then picks among them."""
    sg = _as(np.int64, sigma, -1)
    n6 = NUM_ROUTED_WIRES * degree
    assert sg.shape[0] == n6 and (sg.size == 0 or (0 <= sg.min() and sg.max() < n6)), "sigma maps [6n] to [6n]"
    _, ident = wire_partitions_to_sigma(field, degree, np.arange(n6, dtype=np.uint32), np.arange(n6 + 1, dtype=np.uint32), k_is)
    return _u64(ident.reshape(n6, 4)[sg], NUM_ROUTED_WIRES, degree, 4)


# ---- the Plookup prover's two loops (plookup/src/plookup.rs) ----
def plookup_sorted_multiset(f, t):
    """`s` of the Plookup protocol: f ++ t sorted by t, as sort_by orders it (plookup.rs:171-177, a stable sort on the position of
    an element's FIRST occurrence in t).  f: (n, 4), t: (n + 1, 4) limb arrays -> (2 n + 1, 4).  An element of f that is not in t makes
    the reference's unwrap() panic -> AssertionError here.  Host only: the sort stays on the host."""
    fa, ta = _elems(0, f), _elems(0, t)
    pos = {}
    for i, row in enumerate(ta):
        pos.setdefault(row.tobytes(), i)
    s = np.concatenate([fa, ta])
    try:
        keys = np.fromiter((pos[row.tobytes()] for row in s), dtype=np.int64, count=s.shape[0])
    except KeyError:
        raise AssertionError("called `Option::unwrap()` on a `None` value: an element of f is not in t")
    return _u64(s[np.argsort(keys, kind="stable")])


def _plookup_f_t(field, f, t):
    """t (N, 4), N a power of two, and f_padded: the n = N - 1 values the reference passes get the zero row that is not read
    -> (log N, f (N, 4), t)"""
    ta = _elems(field, t)
    size = ta.shape[0]
    log_size = log2_strict(size)
    fa = _elems(field, f)
    assert fa.shape[0] in (size - 1, size), "f has n or n + 1 rows"
    if fa.shape[0] == size - 1:
        fa = np.concatenate([fa, np.zeros((1, 4), dtype=np.uint64)])
    return log_size, fa, ta


def plookup_sorted_multiset_device(field, f, t):
    """plookup_sorted_multiset through the device (plk_plookup_sorted_multiset; host arrays, copied through PCIe): f (N, 4) = f_padded
    or the n = N - 1 values the reference passes, t (N, 4), N a power of two >= 2 -> (2 N - 1, 4).  An element of f that is not in t
    makes the reference's unwrap() panic -> AssertionError."""
    log_size, fa, ta = _plookup_f_t(field, f, t)
    out = np.empty((2 * ta.shape[0] - 1, 4), dtype=np.uint64)
    missing = ctypes.c_uint(0)
    _call(_lib.load().plk_plookup_sorted_multiset(log_size, field, _ptr(fa), _ptr(ta), _ptr(out), ctypes.byref(missing)),
          "called `Option::unwrap()`", "called `Option::unwrap()` on a `None` value: %d elements of f are not in t" % missing.value)
    return out


def plookup_grand_polynomial(field, f, t, s, beta, gamma, return_closes=False):
    """grand_polynomial (plookup.rs:180-202): f (N, 4) = f_padded (or the n = N - 1 values the reference passes: the last row is not
    read), t (N, 4), s (2 N - 1, 4) -> the N values of Z, values[0] = values[N - 1] = 1.  A zero denominator in rows 0..n-2 panics in
    the reference ("No inverse") -> AssertionError.  return_closes: also whether the product over all n rows is 1 (f is in t)."""
    log_size, fa, ta = _plookup_f_t(field, f, t)
    size = ta.shape[0]
    sa = _elems(field, s)
    assert sa.shape[0] == 2 * size - 1, "s has 2 n + 1 rows"
    b, g = _scalar(beta), _scalar(gamma)
    out = np.empty((size, 4), dtype=np.uint64)
    closes = ctypes.c_int(0)
    # the reference panics (plookup.rs:191, field.rs Div)
    _call(_lib.load().plk_plookup_grand_product(log_size, field, _ptr(fa), _ptr(ta), _ptr(sa), _ptr(b), _ptr(g), _ptr(out), ctypes.byref(closes)), *_NO_INVERSE)
    return (out, bool(closes.value)) if return_closes else out


def plookup_vanishing_values(field, values_4n, alpha, beta, gamma):
    """The 4(n+1)-point loop of vanishing_polynomial (plookup.rs:225-269): values_4n (5, 4 N, 4), rows z, f, t, h1, h2 on the 4N domain
    -> (4 N, 4); Polynomial::from_evaluations of the result is the vanishing polynomial."""
    v = _u64(values_4n)
    assert v.ndim == 3 and v.shape[0] == 5 and v.shape[2] == 4
    log_size = log2_strict(v.shape[1]) - 2
    sc = [_scalar(x) for x in (alpha, beta, gamma)]
    out = np.empty((v.shape[1], 4), dtype=np.uint64)
    _call(_lib.load().plk_plookup_vanishing_points(log_size, field, _ptr(v), *map(_ptr, sc), _ptr(out)))
    return out


# ---- the opening step (plonk.rs:261-308, halo.rs:38-44 and 143-155, plonk_util.rs:123-133 and 311-326) ----
def _poly_args(polys):
    """list of (len, 4) limb arrays -> (kept arrays, ctypes array of host pointers, lengths)"""
    arrs = [_scalars(p) for p in polys]
    lens = np.array([a.shape[0] for a in arrs], dtype=np.uint64)  # size_t
    return arrs, _ptrs(arrs, null_empty=True), lens


def powers(field, x, n):
    """powers (plonk_util.rs:123-133): [1, x, ..., x^(n-1)] as (n, 4)."""
    xs = _scalar(x)
    out = np.empty((n, 4), dtype=np.uint64)
    _call(_lib.load().plk_field_powers(field, _ptr(xs), n, _ptr(out)))
    return out


def eval_polys(field, polys, points):
    """open_all_polynomials (plonk.rs:459-482): out[k][i] = polys[i].eval_from_power(powers(points[k], len(polys[i]))), (n_points, n_polys, 4).
    polys: a list of (len, 4) coefficient arrays of any lengths; 1..8 points."""
    arrs, ptrs, lens = _poly_args(polys)
    pts = _scalars(points)
    out = np.empty((pts.shape[0], len(arrs), 4), dtype=np.uint64)
    _call(_lib.load().plk_plonk_eval_polys(field, len(arrs), ptrs, _ptr(lens), pts.shape[0], _ptr(pts), _ptr(out)))
    return out


def reduce_polynomials(field, polys, scalars, degree):
    """reduced_coeffs of batch_opening_proof (halo.rs:38-44): out[j] = sum_i scalars[i] * polys[i][j], (degree, 4); a polynomial longer
    than `degree` trips the reference's assertion -> AssertionError here."""
    arrs, ptrs, lens = _poly_args(polys)
    sc = _scalars(scalars)
    assert sc.shape[0] == len(arrs), "one scalar per polynomial"
    assert all(a.shape[0] <= degree for a in arrs), "polynomial longer than the degree"
    out = np.empty((degree, 4), dtype=np.uint64)
    _call(_lib.load().plk_poly_reduce(field, len(arrs), ptrs, _ptr(lens), _ptr(sc), degree, _ptr(out)))
    return out


def build_halo_b(field, points, v, degree):
    """build_halo_b (halo.rs:143-155): out[j] = sum_k v^k points[k]^j, (degree, 4)."""
    pts, vs = _scalars(points), _scalar(v)
    out = np.empty((degree, 4), dtype=np.uint64)
    _call(_lib.load().plk_halo_build_b(field, pts.shape[0], _ptr(pts), _ptr(vs), degree, _ptr(out)))
    return out


def halo_s(field, us):
    """halo_s (plonk_util.rs:311-326): the 2^k coefficients of g(X, us).  A zero challenge has no inverse: the reference panics
    ("No inverse", field.rs:266) -> AssertionError here."""
    u = _scalars(us)
    out = np.empty((1 << u.shape[0], 4), dtype=np.uint64)
    _call(_lib.load().plk_halo_s(field, u.shape[0], _ptr(u), _ptr(out)), *_NO_INVERSE)
    return out


# ---- batch inversion (field.rs:223-278, curve.rs:216-232) ----
def batch_multiplicative_inverse(field, x):
    """Field::batch_multiplicative_inverse (field.rs:251-278): panics ("No inverse") on a zero element -> AssertionError here."""
    a = _elems(field, x)
    out = np.empty_like(a)
    _call(_lib.load().plk_field_batch_inverse(field, _ptr(a), _ptr(out), a.shape[0]), *_NO_INVERSE)
    return out


def batch_multiplicative_inverse_opt(field, x):
    """Field::batch_multiplicative_inverse_opt (field.rs:223-249): (inverses, is_none) - zero elements have no inverse."""
    a = _elems(field, x)
    out = np.empty_like(a)
    none = np.zeros(a.shape[0], dtype=np.uint8)
    _call(_lib.load().plk_field_batch_inverse_opt(field, _ptr(a), _ptr(out), _ptr(none), a.shape[0]))
    return out, none


def batch_to_affine(curve, proj_xyz, zero=None):
    """ProjectivePoint::batch_to_affine (curve.rs:216-232): (n, 3, L) homogeneous projective limbs (+ zero flags) -> ((n, 2, L), zero flags)."""
    L = _curve_limbs(curve)
    p = _u64(proj_xyz, -1, 3, L)
    n = p.shape[0]
    z = _u8(zero)
    out = np.empty((n, 2, L), dtype=np.uint64)
    oz = np.zeros(n, dtype=np.uint8)
    _call(_lib.load().plk_curve_batch_to_affine(curve, n, _ptr(p), _ptr(z), _ptr(out), _ptr(oz)))
    return out, oz


# ---- canonical byte encodings (serialization.rs:17-72) ----
def field_to_bytes(field, x):
    """ToBytes for field elements: (n, BYTES) uint8, little-endian canonical value."""
    a = _elems(field, x)
    out = np.empty((a.shape[0], a.shape[1] * 8), dtype=np.uint8)
    _call(_lib.load().plk_field_to_bytes(field, _ptr(a), a.shape[0], _ptr(out)))
    return out


def field_from_bytes(field, b):
    """FromBytes for field elements; "Out of range" (field.rs:100) raises ValueError."""
    L = _field_limbs(field)
    bb = _u8(b, -1, L * 8)
    out = np.empty((bb.shape[0], L), dtype=np.uint64)
    _call(_lib.load().plk_field_from_bytes(field, _ptr(bb), bb.shape[0], _ptr(out)), refusal=True)
    return out


def point_to_bytes(curve, xy, zero=None):
    """ToBytes for AffinePoint: (n, 1 + BYTES) uint8: mask = zero | (y odd) << 1, then x."""
    p = _points(curve, xy)
    z = _u8(zero)
    out = np.empty((p.shape[0], 1 + p.shape[2] * 8), dtype=np.uint8)
    _call(_lib.load().plk_curve_point_to_bytes(curve, _ptr(p), _ptr(z), p.shape[0], _ptr(out)))
    return out


def point_from_bytes(curve, b, with_status=False):
    """FromBytes for AffinePoint: ((n, 2, L), zero flags); an undecodable record raises ValueError unless with_status."""
    L = _curve_limbs(curve)
    bb = _u8(b, -1, 1 + L * 8)
    n = bb.shape[0]
    out = np.empty((n, 2, L), dtype=np.uint64)
    oz = np.zeros(n, dtype=np.uint8)
    st = np.zeros(n, dtype=np.uint8)
    rc = _lib.load().plk_curve_point_from_bytes(curve, _ptr(bb), n, _ptr(out), _ptr(oz), _ptr(st))
    if with_status and rc in (_lib.PLK_OK, _lib.PLK_ERR_INVALID_ARG):
        return out, oz, st
    _call(rc, refusal=True)
    return out, oz


# ---- Pedersen generators: the BLAKE3 hash to the curve (hash_to_curve.rs:13-76) ----
def blake_field(field, iters, seeds):
    """blake_field(iter, seed) per row: seeds (n, L) Montgomery limbs, iters a u8 per row (or one for all).  Returns (x (n, L), y_neg (n,))."""
    a = _elems(field, seeds)
    it = _u8(np.broadcast_to(np.asarray(iters, dtype=np.uint8), (a.shape[0],)))
    x = np.empty_like(a)
    y_neg = np.zeros(a.shape[0], dtype=np.uint8)
    _call(_lib.load().plk_blake_field(a.shape[0], field, _ptr(it), _ptr(a), _ptr(x), _ptr(y_neg)), refusal=True)
    return x, y_neg


def blake_hash_base_field_to_curve(curve, seeds):
    """blake_hash_base_field_to_curve::<C>(seed) per row of seeds ((n, L) Montgomery limbs of the base field): (n, 2, L) affine points."""
    a = _elems(CURVE_BASE_FIELD[curve], seeds)
    out = np.empty((a.shape[0], 2, a.shape[1]), dtype=np.uint64)
    _call(_lib.load().plk_hash_field_to_curve(a.shape[0], curve, _ptr(a), _ptr(out)), refusal=True)
    return out


def blake_hash_usize_to_curve(curve, seed, count=None):
    """blake_hash_usize_to_curve::<C>(seed): (2, L); with count, the points of seed .. seed + count - 1: (count, 2, L)."""
    n = 1 if count is None else int(count)
    out = np.empty((n, 2, _curve_limbs(curve)), dtype=np.uint64)
    _call(_lib.load().plk_hash_to_curve(n, curve, int(seed), _ptr(out)), refusal=True)
    return out[0] if count is None else out


def pedersen_generators(curve, degree):
    """circuit_builder.rs:1127-1129: (g[0 .. degree), h = the point of seed degree, u = the point of seed degree + 1)."""
    pts = blake_hash_usize_to_curve(curve, 0, degree + 2)
    return pts[:degree], pts[degree], pts[degree + 1]


# ---- Rescue: the permutation, the sponge, k-th roots and the Challenger (rescue.rs, mds.rs, field.rs:340-375, plonk_challenger.rs) ----
RESCUE_SPONGE_WIDTH, RESCUE_SPONGE_RATE = 4, 3


def rescue_rounds(width, security_bits):
    """recommended_rounds (rescue.rs:123-125)."""
    r = ctypes.c_size_t(0)
    _call(_lib.load().plk_rescue_rounds(int(width), int(security_bits), ctypes.byref(r)), refusal=True)
    return int(r.value)


def rescue_mds(field, width=RESCUE_SPONGE_WIDTH):
    """mds_matrix::<F>(width) (mds.rs:56-77): (width, width, L) Montgomery limbs."""
    out = np.empty((width, width, _field_limbs(field, strict=False)), dtype=np.uint64)
    _call(_lib.load().plk_rescue_mds(int(width), field, _ptr(out)), refusal=True)
    return out


class RescueContext:
    """What rescue_permutation needs besides the state: field, width, rounds and, on the device, the round constants, the MDS matrix
    and the exponent of 1 / ALPHA.  constants: (rounds, 2, width, L) Montgomery limbs, step A then step B per round, as
    generate_rescue_constants (rescue.rs:97-121) returns them - the caller brings them (the reference draws them from
    ChaCha8Rng::seed_from_u64(1337), which is not restated here)."""

    def __init__(self, field, constants, width=RESCUE_SPONGE_WIDTH, rounds=None):
        L = _field_limbs(field, strict=False)
        c = _u64(constants)
        if rounds is None:
            rounds = c.size // (2 * width * L) if width else 0
        assert c.size == rounds * 2 * width * L, "constants: rounds x 2 x width elements"
        self.field, self.width, self.rounds = field, int(width), int(rounds)
        self._ctx = ctypes.c_void_p()
        _call(_lib.load().plk_rescue_create(self.width, field, self.rounds, _ptr(c), ctypes.byref(self._ctx)), refusal=True)

    @property
    def handle(self):
        assert self._ctx is not None and self._ctx.value, "the context has been freed"
        return self._ctx

    def free(self):
        if self._ctx is not None and self._ctx.value:
            _call(_lib.load().plk_rescue_free(self._ctx))
        self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def rescue_permutation(ctx, states):
    """rescue_permutation (rescue.rs:70-88) per state: (n, 4, L) or (4, L) Montgomery limbs -> the same shape."""
    a = _u64(states)
    L = _field_limbs(ctx.field)
    assert a.shape[-2:] == (ctx.width, L)
    out = np.empty_like(a)
    _call(_lib.load().plk_rescue_permutation(a.size // (ctx.width * L), ctx.handle, _ptr(a), _ptr(out)), refusal=True)
    return out


def rescue_sponge(ctx, inputs, num_outputs):
    """rescue_sponge (rescue.rs:40-68) per row: inputs (n, n_inputs, L) or (n_inputs, L) -> (n, num_outputs, L) or (num_outputs, L)."""
    L = _field_limbs(ctx.field)
    a = _u64(inputs)
    single = a.ndim == 2
    a = a.reshape((1,) + a.shape) if single else a
    assert a.ndim == 3 and a.shape[2] == L
    out = np.empty((a.shape[0], int(num_outputs), L), dtype=np.uint64)
    _call(_lib.load().plk_rescue_sponge(a.shape[0], ctx.handle, a.shape[1], _ptr(a), int(num_outputs), _ptr(out)), refusal=True)
    return out[0] if single else out


# ---- gate witness rows (include/plonky_hip_trace.h): the blocks of the in-circuit Rescue permutation and of curve_msm ----
TRACE_NONE = 0xFFFFFFFF  # status word [2] when no instance met an exceptional case


def _trace_tables(n_rows, count, first_rows, wires, constants):
    """the caller's tables as the entries take them: wires (9, n_rows, 4), fresh zeros when None; constants None (not written), True
    (fresh zeros) or the caller's (6, n_rows, 4); first_rows (count,) uint32; four status words"""
    assert wires is None or np.shape(wires) == (NUM_WIRES, n_rows, 4), "wires: (9, n_rows, 4)"
    assert constants is None or constants is True or np.shape(constants) == (NUM_CONSTANTS, n_rows, 4), "constants: (6, n_rows, 4)"
    assert np.size(first_rows) == count, "first_rows: one row per instance"
    w = np.zeros((NUM_WIRES, n_rows, 4), dtype=np.uint64) if wires is None else _u64(wires, NUM_WIRES, n_rows, 4)
    k = np.zeros((NUM_CONSTANTS, n_rows, 4), dtype=np.uint64) if constants is True else None if constants is None else _u64(constants, NUM_CONSTANTS, n_rows, 4)
    return w, k, _as(np.uint32, first_rows, count), np.zeros(4, dtype=np.uint32)


def trace_rescue_permutation(ctx, inputs, n_rows, first_rows, wires=None, constants=None):
    """The rows CircuitBuilder::rescue_permutation lays down (circuit_builder.rs:931-970), as RescueStepAGate / RescueStepBGate generate
    them, per instance: inputs (count, 4, 4) Montgomery limbs, first_rows (count,) the first row of each block of 2 rounds + 1 rows.
    wires: the caller's wire_values_by_wire_index (9, n_rows, 4), written in place where it is a contiguous uint64 array (None: a
    fresh table of zeros); constants: None, True (a fresh table) or the caller's (6, n_rows, 4) - the blocks' gate constants are then
    written too.  Returns (wires, constants, status): status (4,) uint32, [0] blocks that would pass n_rows (not written)."""
    a = _u64(inputs)
    assert a.ndim == 3 and a.shape[1:] == (RESCUE_SPONGE_WIDTH, 4), "inputs: (count, 4, 4)"
    w, k, fr, st = _trace_tables(n_rows, a.shape[0], first_rows, wires, constants)
    _call(_lib.load().plk_trace_rescue_permutation(a.shape[0], ctx.handle, _ptr(a), n_rows, _ptr(w), _ptr(fr), _ptr(k), _ptr(st)), refusal=True)
    return w, k, st


def trace_curve_msm(curve, points, scalars, start, n_bits, n_rows, first_rows, wires=None, constants=None):
    """The rows CircuitBuilder::curve_msm lays down (circuit_curve.rs:287-410) per instance: points (count, parts, 2, 4) affine points
    of the INNER curve, scalars (count, parts, 4) elements of its base field (part.scalar.convert()), start (2, 4) the starting
    accumulator, n_bits the bits of the chain (the builder's BITS - 1); a block is n_bits (parts + 1) rows.  Tables and result as
    trace_rescue_permutation; status [1] counts the instances that met an exceptional case.  AssertionError where the reference
    panics ("x_1 = x_2", "y = 0"), ValueError for a scalar with a bit at or above n_bits: the tables are written all the same."""
    pts = _u64(points)
    assert pts.ndim == 4 and pts.shape[2:] == (2, 4), "points: (count, parts, 2, 4)"
    count, parts = pts.shape[:2]
    sc = _u64(scalars)
    assert sc.shape == (count, parts, 4), "scalars: (count, parts, 4)"
    w, k, fr, st = _trace_tables(n_rows, count, first_rows, wires, constants)
    _call(_lib.load().plk_trace_curve_msm(count, parts, int(n_bits), curve, _ptr(pts), _ptr(sc), _ptr(_u64(start, 2, 4)), n_rows, _ptr(w), _ptr(fr), _ptr(k),
                                          _ptr(st)), panics=("x_1 = x_2", "y = 0"), refusal=True)
    return w, k, st


# ---- the Rescue hash to the curve (hash_to_curve.rs:3-11, 78-104); ctx: a RescueContext over the curve's base field ----
def hash_base_field_to_curve(ctx, curve, seeds):
    """hash_base_field_to_curve::<C>(seed, security_bits) per row of seeds ((n, L) or (L,) Montgomery limbs of the base field), the
    context's rounds standing for security_bits: (n, 2, L) or (2, L) affine points."""
    a = _u64(seeds)
    single = a.ndim == 1
    a = _elems(CURVE_BASE_FIELD[curve], a.reshape(1, -1) if single else a)
    out = np.empty((a.shape[0], 2, a.shape[1]), dtype=np.uint64)
    _call(_lib.load().plk_rescue_hash_field_to_curve(a.shape[0], ctx.handle, curve, _ptr(a), _ptr(out)), refusal=True)
    return out[0] if single else out


def hash_usize_to_curve(ctx, curve, seed, count=None):
    """hash_usize_to_curve::<C>(seed, security_bits): (2, L); with count, the points of seed .. seed + count - 1: (count, 2, L)."""
    n = 1 if count is None else int(count)
    out = np.empty((n, 2, _curve_limbs(curve, strict=False)), dtype=np.uint64)
    _call(_lib.load().plk_rescue_hash_to_curve(n, ctx.handle, curve, int(seed), _ptr(out)), refusal=True)
    return out[0] if count is None else out


def hash_u32_to_curve(ctx, curve, seed, count=None):
    """hash_u32_to_curve::<C>(seed, security_bits): hash_usize_to_curve over seeds that fit a u32."""
    last = int(seed) + (1 if count is None else int(count)) - 1
    if int(seed) < 0 or last >= 1 << 32:
        raise ValueError("seeds %d .. %d do not fit a u32" % (int(seed), last))
    return hash_usize_to_curve(ctx, curve, seed, count)


def rescue_hash_n_to_1(ctx, inputs):  # rescue.rs:26-28
    return rescue_sponge(ctx, inputs, 1)


def rescue_hash_n_to_2(ctx, inputs):  # rescue.rs:30-33
    return rescue_sponge(ctx, inputs, 2)


def rescue_hash_n_to_3(ctx, inputs):  # rescue.rs:35-38
    return rescue_sponge(ctx, inputs, 3)


def kth_root(field, x, k):
    """Field::kth_root_u32(k) (field.rs:340-375) per element of x ((n, L) Montgomery limbs); ValueError where the reference panics."""
    a = _u64(x)
    out = np.empty_like(a)
    _call(_lib.load().plk_field_kth_root(a.size // _field_limbs(field, strict=False), field, int(k), _ptr(a), _ptr(out)), refusal=True)
    return out


class Challenger:
    """Challenger<F> (plonk_challenger.rs:20-109) over a RescueContext; elements are (L,) arrays of Montgomery limbs.  Every
    permutation is one rescue_permutation call of count 1: a transcript is a latency chain, the device pays for batches.

    The mirror is literal, including two things the reference does that a reader may take for slips and that are NOT repaired here:
    get_challenge pops from the END of the output buffer (state[2] first), and absorb_buffered_inputs refills the output buffer
    from state[0..3] on every call, also with nothing buffered - so challenges drawn with no observation in between are the same
    element (get_2_challenges returns two equal values)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.sponge_state = np.zeros((RESCUE_SPONGE_WIDTH, _field_limbs(ctx.field)), dtype=np.uint64)
        self.input_buffer = []
        self.output_buffer = []

    def clone(self):
        c = Challenger(self.ctx)
        c.sponge_state = self.sponge_state.copy()
        c.input_buffer = [e.copy() for e in self.input_buffer]
        c.output_buffer = [e.copy() for e in self.output_buffer]
        return c

    def observe_element(self, element):
        self.output_buffer = []
        self.input_buffer.append(np.array(element, dtype=np.uint64).reshape(_field_limbs(self.ctx.field)))

    def observe_elements(self, elements):
        for e in elements:
            self.observe_element(e)

    def observe_affine_point(self, point):
        """point: (2, L), x then y (the reference asserts it is not the identity)"""
        self.observe_element(point[0])
        self.observe_element(point[1])

    def observe_affine_points(self, points):
        for pt in points:
            self.observe_affine_point(pt)

    def get_challenge(self):
        self._absorb_buffered_inputs()
        if not self.output_buffer:  # plonk_challenger.rs:66-70; never taken, the buffer has just been filled
            self.sponge_state = rescue_permutation(self.ctx, self.sponge_state)
            self.output_buffer = [self.sponge_state[i].copy() for i in range(RESCUE_SPONGE_RATE)]
        return self.output_buffer.pop()

    def get_2_challenges(self):
        return self.get_challenge(), self.get_challenge()

    def get_3_challenges(self):
        return self.get_challenge(), self.get_challenge(), self.get_challenge()

    def get_n_challenges(self, n):
        return [self.get_challenge() for _ in range(n)]

    def _absorb_buffered_inputs(self):
        for at in range(0, len(self.input_buffer), RESCUE_SPONGE_RATE):
            chunk = np.stack(self.input_buffer[at:at + RESCUE_SPONGE_RATE])
            self.sponge_state[:len(chunk)] = field_op(self.ctx.field, "add", self.sponge_state[:len(chunk)], chunk)
            self.sponge_state = rescue_permutation(self.ctx, self.sponge_state)
        self.output_buffer = [self.sponge_state[i].copy() for i in range(RESCUE_SPONGE_RATE)]
        self.input_buffer = []


# ---- a point times a scalar of its own, the Halo endomorphism and the group side of the verifier ----
# (curve_multiplication.rs:5-85, plonk_util.rs:50-110 / 329-339, halo.rs:157-223, verifier.rs:173-186)
def _scalar_mul_args(curve, scalars, points, zero):
    s, p, z = _scalars(scalars), _points(curve, points), _u8(zero, -1)
    assert z is None or z.shape[0] == p.shape[0]
    count = max(s.shape[0], p.shape[0])
    return s, p, z, count, np.zeros((count, 2, p.shape[2]), dtype=np.uint64), np.zeros(count, dtype=np.uint8)


def curve_scalar_mul(curve, scalars, points, zero=None):
    """CurveScalar * ProjectivePoint per element: out_i = [s_i] P_i.  scalars (n, 4) or (4,) Montgomery limbs in the curve's scalar
    field, points (n, 2, L) or (2, L) affine; a single scalar or a single point is broadcast.  Returns (points (n, 2, L), zero flags)."""
    s, p, z, count, out, oz = _scalar_mul_args(curve, scalars, points, zero)
    _call(_lib.load().plk_curve_scalar_mul(count, curve, s.shape[0], _ptr(s), p.shape[0], _ptr(p), _ptr(z), _ptr(out), _ptr(oz)), refusal=True)
    return out, oz


def halo_n(curve, scalars, security_bits=128):
    """halo_n (plonk_util.rs:50-75) of to_canonical_bool_vec()[..security_bits] per scalar: (n, 4) Montgomery limbs, scalar field."""
    s = _scalars(scalars)
    out = np.empty_like(s)
    _call(_lib.load().plk_halo_n(s.shape[0], curve, int(security_bits), _ptr(s), _ptr(out)), refusal=True)
    return out


def halo_n_mul(curve, scalars, points, zero=None, security_bits=128):
    """halo_n_mul (plonk_util.rs:79-110) per element: [n(s_i)] P_i by Algorithm 1; shapes and broadcast as curve_scalar_mul."""
    s, p, z, count, out, oz = _scalar_mul_args(curve, scalars, points, zero)
    _call(_lib.load().plk_halo_n_mul(count, curve, int(security_bits), s.shape[0], _ptr(s), p.shape[0], _ptr(p), _ptr(z), _ptr(out), _ptr(oz)),
          refusal=True)
    return out, oz


def halo_g(field, x, us):
    """halo_g (plonk_util.rs:329-339): g(x, us) = prod over us REVERSED of (u_i x^(2^j) + u_i^-1).  log n products: host-driven."""
    u = _scalars(us)
    product = powers(field, x, 1)[0:1]  # ONE
    x_power = _u64(x, 1, 4)
    for i in range(u.shape[0] - 1, -1, -1):
        u_i = u[i:i + 1]
        term = field_op(field, "add", field_op(field, "mul", u_i, x_power), field_op(field, "inverse", u_i))
        product = field_op(field, "mul", product, term)
        x_power = field_op(field, "square", x_power)
    return product[0]


def _point(curve, p):
    """a point argument: (2, L) limbs, or (limbs, zero flag)"""
    if isinstance(p, tuple):
        return _points(curve, p[0])[0], int(np.asarray(p[1]).reshape(-1)[0])
    return _points(curve, p)[0], 0


def _point_sum(curve, pts):
    return curve_sum_affine(curve, np.stack([p[0] for p in pts]), np.array([p[1] for p in pts], dtype=np.uint8))


def _blinded(sf, a, c, d):
    """a c + d in the scalar field: the z of a Schnorr proof"""
    return field_op(sf, "add", field_op(sf, "mul", _u64(a, 1, 4), c), _u64(d, 1, 4))[0]


def schnorr_protocol(curve, halo_a, halo_b, halo_g, randomness, u_prime, pedersen_h, d, s, challenge):
    """schnorr_protocol (halo.rs:157-182) with the nonces d, s and the challenge as arguments: R = [d](G + [b] U') + [s] H,
    z1 = a c + d, z2 = randomness c + s.  Returns ((R limbs, zero flag), z1, z2)."""
    sf = int(_lib.load().plk_curve_scalar_field(curve))
    g, up, h = _point(curve, halo_g), _point(curve, u_prime), _point(curve, pedersen_h)
    bu, buz = curve_scalar_mul(curve, halo_b, up[0], [up[1]])
    gu = _point_sum(curve, [g, (bu[0], int(buz[0]))])
    m, mz = curve_scalar_mul(curve, np.stack([_scalar(d), _scalar(s)]), np.stack([gu[0], h[0]]), [gu[1], h[1]])
    r = _point_sum(curve, [(m[0], int(mz[0])), (m[1], int(mz[1]))])
    c = _u64(challenge, 1, 4)
    return r, _blinded(sf, halo_a, c, d), _blinded(sf, randomness, c, s)


def verify_ipa(curve, halo_l, halo_r, halo_g, commitment, value, halo_b, halo_us, u_prime, pedersen_h, schnorr_challenge, schnorr_proof):
    """verify_ipa (halo.rs:186-223).  halo_l / halo_r: (k, 2, L) affine points (or (points, zero flags)); the other points (2, L) or
    (limbs, zero flag); scalars (4,) Montgomery limbs; schnorr_proof = (R, z1, z2).  P' = C + [value] U',
    Q = <u^2, L> + <u^-2, R> + P', and the check is [c] Q + R == [z1](G + [b] U') + [z2] H on unique affine points."""
    sf = int(_lib.load().plk_curve_scalar_field(curve))
    us = _scalars(halo_us)
    lr, lrz = [], []
    for side in (halo_l, halo_r):
        pts, flags = side if isinstance(side, tuple) else (side, None)
        pts = _points(curve, pts)
        assert pts.shape[0] == us.shape[0], "one L_j and one R_j per challenge"
        lr.append(pts)
        lrz.append(np.zeros(pts.shape[0], dtype=np.uint8) if flags is None else _u8(flags, -1))
    g, com, up, h = _point(curve, halo_g), _point(curve, commitment), _point(curve, u_prime), _point(curve, pedersen_h)
    r, z1, z2 = schnorr_proof
    r = _point(curve, r)
    # [value] U' and [b] U': one call, two scalars over the one point
    t, tz = curve_scalar_mul(curve, np.stack([_scalar(value), _scalar(halo_b)]), up[0], [up[1]])
    p_prime = _point_sum(curve, [com, (t[0], int(tz[0]))])
    scalars = np.concatenate([field_op(sf, "square", us), field_op(sf, "square", field_op(sf, "inverse", us))])
    q = msm_parallel(curve, scalars, np.concatenate(lr), 8, zero=np.concatenate(lrz))
    q = _point_sum(curve, [q, p_prime])
    gu = _point_sum(curve, [g, (t[1], int(tz[1]))])
    m, mz = curve_scalar_mul(curve, np.stack([_scalar(schnorr_challenge), _scalar(z1), _scalar(z2)]), np.stack([q[0], gu[0], h[0]]), [q[1], gu[1], h[1]])
    lhs = _point_sum(curve, [(m[0], int(mz[0])), r])
    rhs = _point_sum(curve, [(m[1], int(mz[1])), (m[2], int(mz[2]))])
    return lhs[1] == rhs[1] and bool(np.array_equal(lhs[0], rhs[0]))


def verify_halo_g(curve, halo_g, halo_us, precomputation):
    """The linear-time G check of the verifier (verifier.rs:173-186): halo_g == <halo_s(us), G> over the caller's tables of the
    2^len(us) generators (an MsmPrecomputation)."""
    sf = int(_lib.load().plk_curve_scalar_field(curve))
    s = halo_s(sf, halo_us)
    assert s.shape[0] == precomputation.n, "2^len(halo_us) generators"
    got = msm_execute_parallel(precomputation, s)
    g = _point(curve, halo_g)
    return got[1] == g[1] and bool(np.array_equal(got[0], g[0]))
