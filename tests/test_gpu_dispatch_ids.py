"""GPU tests of the field / curve dispatch (dispatch.cuh, ec.cuh): what every public entry point that takes a `field` or `curve` id does
with an id outside the range, and that every id inside it still reaches its instantiation.

No kernel is launched by the refusals: each call is made with small, otherwise valid arguments (one pinned buffer that host and device can
both address, so that a site that did launch would do no harm) and must come back with PLK_ERR_INVALID_ARG and the error text the entry
point had before the dispatchers were introduced.  The expectations below come from the commit before them (6a7053a), not from the code
under test: every entry point refused every one of these ids there.  Where an entry point looks at the id before it selects the device,
the return code and text were recorded by calling that commit's library; the twelve that select the device first (plk_ntt_precompute,
plk_ntt_dev, plk_ntt_padded_dev, plk_poly_divide_by_z_h_dev, plk_poly_mul_dev, plk_plonk_vanishing_points_dev, plk_field_op,
plk_field_inner_product_dev, plk_field_fold_slices_dev, plk_curve_batch_to_affine_dev, plk_curve_fold_pairs_dev, plk_curve_fold_multi_dev)
have the text of that commit's source.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from plonky_amd import lib as plk

BAD_FIELDS = (-1, 6, 1000)
BAD_CURVES = (-1, 5, 1000)

# argument codes after the id: P the shared buffer, A an array of four pointers into it, S the null stream, T no tables, integers as they are
P, A, S, T = "P", "A", "S", "T"
# entry point -> (arguments after the id, leading words of plk_last_error(), %d the id)
NO_NTT, NOT_SCALAR, NOT_4, BAD_F, BAD_C = ("field %d has no NTT entry point", "field %d is not a circuit scalar field", "field %d is not a 4-limb field",
                                           "bad field id %d", "bad curve id %d")
FIELD_CALLS = {
    "plk_ntt_precompute": ((2,), NO_NTT),
    "plk_ntt_precompute_table": ((2, P), BAD_F),
    "plk_ntt_precompute_table_dev": ((2, P, S), BAD_F),
    "plk_ntt": ((2, 0, P, P), BAD_F),
    "plk_ntt_batch": ((2, 0, 2, A, A), BAD_F),
    "plk_ntt_dev": ((2, 0, 1, P, P, S), NO_NTT),
    "plk_ntt_padded": ((2, P, 3, P), BAD_F),
    "plk_ntt_padded_batch": ((2, 2, A, P, A), BAD_F),
    "plk_ntt_padded_dev": ((2, 1, P, 3, 4, P, S), NO_NTT),
    "plk_poly_divide_by_z_h": ((P, 4, 2, P, 8, P), NO_NTT),
    "plk_poly_divide_by_z_h_dev": ((P, 4, 2, P, 8, P, S), NO_NTT),
    "plk_poly_mul": ((P, 2, P, 2, P, 8, P), NO_NTT),
    "plk_poly_mul_dev": ((P, 2, P, 2, P, 8, P, S), NO_NTT),
    "plk_poly_division_dev": ((P, 4, P, 2, P, 4, P, S), NOT_4),
    "plk_poly_division": ((P, 4, P, 2, P, 4, P), NOT_4),
    "plk_poly_from_roots": ((2, P, P), NOT_4),
    "plk_plonk_vanishing_points_dev": ((1, P, P, P, P, P, P, P, P, P, P, P, S), NOT_SCALAR),
    "plk_plonk_vanishing_points": ((1, P, P, P, P, P, P, P, P, P, P, P), NOT_SCALAR),
    "plk_plonk_permutation_z_dev": ((1, P, P, 1, P, P, P, P, P, S), NOT_SCALAR),
    "plk_plonk_permutation_z": ((1, P, P, 1, P, P, P, P, P), NOT_SCALAR),
    "plk_plonk_evaluate_all_constraints": ((1, P, P, P, P, P, P, P), NOT_SCALAR),
    "plk_field_powers_dev": ((P, 4, P, S), NOT_4),
    "plk_field_powers": ((P, 4, P), NOT_4),
    "plk_plonk_eval_polys_dev": ((2, A, P, 1, P, P, S), NOT_4),
    "plk_plonk_eval_polys": ((2, A, P, 1, P, P), NOT_4),
    "plk_poly_reduce_dev": ((2, A, P, P, 4, P, S), NOT_4),
    "plk_poly_reduce": ((2, A, P, P, 4, P), NOT_4),
    "plk_halo_build_b_dev": ((2, P, P, 4, P, S), NOT_4),
    "plk_halo_build_b": ((2, P, P, 4, P), NOT_4),
    "plk_halo_s_dev": ((2, P, P, S), NOT_4),
    "plk_halo_s": ((2, P, P), NOT_4),
    "plk_field_batch_inverse": ((P, P, 4), BAD_F),
    "plk_field_batch_inverse_opt": ((P, P, P, 4), BAD_F),
    "plk_field_batch_inverse_dev": ((P, P, P, 4, S), BAD_F),
    "plk_field_to_bytes": ((P, 4, P), BAD_F),
    "plk_field_from_bytes": ((P, 4, P), BAD_F),
    "plk_field_inner_product_dev": ((P, P, 4, P, S), BAD_F),
    "plk_field_fold_slices_dev": ((P, P, P, P, 4, P, S), BAD_F),
    "plk_field_op": ((2, P, P, P, 4), BAD_F),
}
CURVE_CALLS = {
    "plk_msm_precompute": ((4, P, P, 0, P), BAD_C),
    "plk_msm_precompute_dev": ((4, P, P, 0, S, P), BAD_C),
    "plk_msm_precompute_ex": ((4, P, P, 0, 0, P), BAD_C),
    "plk_msm_precompute_dev_ex": ((4, P, P, 0, 0, S, P), BAD_C),
    "plk_msm": ((4, P, P, P, P, P), BAD_C),
    "plk_curve_sum_affine": ((3, P, P, P, P), BAD_C),
    "plk_msm_combine_partials_dev": ((1, 1, 0, P, P, P, S), BAD_C),
    "plk_msm_precompute_table": ((2, P, P, 8, P, P), BAD_C),
    "plk_msm_precompute_table_dev": ((2, P, P, 8, P, P, S), BAD_C),
    "plk_curve_fold_pairs": ((2, P, P, P, P, P, P, P, P), BAD_C),
    "plk_curve_fold_pairs_dev": ((2, P, P, P, P, P, P, P, P, S), BAD_C),
    "plk_curve_batch_to_affine": ((2, P, P, P, P), BAD_C),
    "plk_curve_batch_to_affine_dev": ((2, P, P, P, P, S), BAD_C),
    "plk_curve_point_to_bytes": ((P, P, 2, P), BAD_C),
    "plk_curve_point_from_bytes": ((P, 2, P, P, P), BAD_C),
    "plk_curve_fold_multi_dev": ((2, 1, P, P, P, P, P, S), BAD_C),
    "plk_halo_begin_dev": ((4, P, P, P, P, P, P, 0, S, P), BAD_C),
    # (tables are a context, which only kernels can build: without one the entry point says so before it looks at the curve)
    "plk_halo_begin_tabled_dev": ((4, P, P, P, P, T, P, P, 0, 0, P, 0, 0, S, P), "null tables"),
    "plk_halo_begin": ((4, P, P, P, P, P, P, 0, P), BAD_C),
    "plk_selftest_quad": ((P, 4, 4, P), BAD_C),
    "plk_curve_op": ((0, 0, 4, P, P, P, P, P, P, P, P, P, P), BAD_C),
    "plk_msm_debug_digits": ((8, 4, P, P, P), BAD_C),
    "plk_curve_gen_bases_dev": ((4, 0, P, P, P, S), BAD_C),
}

FIELD_LIMBS = {0: 4, 1: 4, 2: 4, 3: 6, 4: 4, 5: 4}
CURVE_LIMBS = {0: 4, 1: 4, 2: 6, 3: 4, 4: 4}
CURVE_SCALAR_FIELD = {0: 1, 1: 0, 2: 2, 3: 5, 4: 4}
SCALAR_BITS = {0: 255, 1: 255, 2: 253, 3: 255, 4: 255}
TABLE_WINDOWS = (1, 8, 13, 64)


@pytest.fixture(scope="module")
def L():
    from plonky_amd import device as dev
    dev.init(0)
    return plk.load()


@pytest.fixture(scope="module")
def buffers():
    """64 KiB of pinned memory holding the stored word 1 in every 64-bit limb (non-zero elements, lengths of 1), and four pointers to it"""
    import torch
    buf = torch.ones(8192, dtype=torch.int64).pin_memory()
    ptrs = torch.full((4,), buf.data_ptr(), dtype=torch.int64).pin_memory()
    return buf, ptrs


def call(L, buffers, name, ident, spec):
    buf, ptrs = buffers
    args = [{P: buf.data_ptr(), A: ptrs.data_ptr(), S: None, T: None}.get(a, a) if isinstance(a, str) else a for a in spec]
    rc = getattr(L, name)(ident, *args)
    return rc, L.plk_last_error().decode("utf-8", "replace")


def test_every_entry_point_is_listed():
    """the tables above name every declared function whose first argument is a field or curve id (the id -> property functions apart)"""
    ids_first = {n for n, _, a in plk.SYMBOLS if a and a[0] is ctypes.c_int and n not in (
        "plk_init", "plk_init_devices", "plk_set_thread_device", "plk_thread_hip_device", "plk_ntt_set_profiling")}
    props = {"plk_field_limbs", "plk_curve_limbs", "plk_curve_scalar_field", "plk_msm_table_digits", "plk_msm_partials_bytes"}
    assert ids_first - props == set(FIELD_CALLS) | set(CURVE_CALLS)


@pytest.mark.parametrize("name", sorted(FIELD_CALLS))
def test_unknown_field_is_refused(L, buffers, name):
    spec, text = FIELD_CALLS[name]
    for ident in BAD_FIELDS:
        rc, err = call(L, buffers, name, ident, spec)
        print(name, ident, rc, repr(err))
        assert rc == plk.PLK_ERR_INVALID_ARG and err.startswith(text % ident), (name, ident, rc, err)


@pytest.mark.parametrize("name", sorted(CURVE_CALLS))
def test_unknown_curve_is_refused(L, buffers, name):
    spec, text = CURVE_CALLS[name]
    for ident in BAD_CURVES:
        rc, err = call(L, buffers, name, ident, spec)
        print(name, ident, rc, repr(err))
        assert rc == plk.PLK_ERR_INVALID_ARG and err.startswith(text % ident if "%" in text else text), (name, ident, rc, err)


def test_id_properties(L):
    for i in range(-2, 9):
        assert L.plk_field_limbs(i) == FIELD_LIMBS.get(i, plk.PLK_ERR_INVALID_ARG), i
        assert L.plk_curve_limbs(i) == CURVE_LIMBS.get(i, plk.PLK_ERR_INVALID_ARG), i
        assert L.plk_curve_scalar_field(i) == CURVE_SCALAR_FIELD.get(i, plk.PLK_ERR_INVALID_ARG), i
        for w in TABLE_WINDOWS:
            exp = (SCALAR_BITS[i] + w - 1) // w if i in SCALAR_BITS else plk.PLK_ERR_INVALID_ARG
            assert L.plk_msm_table_digits(i, w) == exp, (i, w)
        assert L.plk_msm_table_digits(i, 0) == plk.PLK_ERR_INVALID_ARG, i
        assert L.plk_msm_partials_bytes(i, 2) == ((2 * 2 * CURVE_LIMBS[i] * 8 + 2 + 15) & ~15 if i in CURVE_LIMBS else 0), i


# ---- every valid id still reaches its instantiation ----
@pytest.mark.parametrize("f", list(br.FIELDS.values()), ids=lambda f: f.name)
def test_field_op_every_field(L, f):
    from plonky_amd import api
    a, b = ol.rand_field(f.field_id, 0xD15 + f.field_id, 4), ol.rand_field(f.field_id, 0xD16 + f.field_id, 4)
    assert np.array_equal(api.field_op(f.field_id, "mul", a, b), ol.field_binop(f.field_id, "mul", a, b))


@pytest.mark.parametrize("c", list(br.CURVES.values()), ids=lambda c: c.name)
def test_curve_sum_affine_every_curve(L, c):
    import plonky_amd as pa
    G = (c.gx, c.gy)
    pts = np.array([[c.base.mont_limbs(Q[0]), c.base.mont_limbs(Q[1])] for Q in (G, br.ec_mul(c, 5, G), br.ec_mul(c, 11, G))],
                   dtype=np.uint64).reshape(3, 2, c.base.n_limbs)
    out, z = pa.curve_sum_affine(c.curve_id, pts)
    exp, ez = ol.affine_summation(c.curve_id, "best", pts)
    assert z == ez == 0 and np.array_equal(out, exp)


@pytest.mark.parametrize("f", [f for f in br.FIELDS.values() if f.n_limbs == 4], ids=lambda f: f.name)
def test_halo_s_every_scalar_field(L, f):
    """plk_halo_s with two challenges against the reference's loop (plonk_util.rs:311-326), as tests/test_gpu_opening.py writes it"""
    from plonky_amd import api
    from tests.test_gpu_opening import ref_halo_s, scalar_words, words_to_ints
    us = [f.p - 1, 0x1234567 + f.field_id]
    assert words_to_ints(api.halo_s(f.field_id, scalar_words(f, us))) == ref_halo_s(f, us)
