"""The argument checks of the C ABI's wrappers (plonky_amd/csrc/capi.hip) that return BEFORE any device call: one case per refusal
branch and per `count == 0 -> PLK_OK` return, as (label, entry, arguments).  tests/golden/capi_refusals.json holds what each case
returned - (code, plk_last_error() text) - from the library as it was before the wrappers were reworked; tests/test_capi_refusals.py
asserts the same pairs.  Nothing here reaches ensure_device(): its text depends on the machine, and the texts of failed HIP calls
carry file and line.

    python tests/capi_refusal_cases.py OUT.json        records the pairs from the library lib.SO_PATH (PLK_HIP_LIB) names
"""
import ctypes
import json
import os
import sys

import numpy as np

B = np.ones(4096, dtype=np.uint64)     # any readable buffer: non-zero limbs (a non-zero h[0], leading coefficient, challenge)
Z = np.zeros(4096, dtype=np.uint64)    # zero limbs where a check reads them
W = np.ones(16, dtype=np.uint64)       # where a case that gets past its checks writes a count
b, z, w = B.ctypes.data, Z.ctypes.data, W.ctypes.data
_keep = []


def ptrs(*vals):
    a = (ctypes.c_void_p * len(vals))(*vals)
    _keep.append(a)
    return ctypes.addressof(a)


def sizes(*vals):
    a = (ctypes.c_size_t * len(vals))(*vals)
    _keep.append(a)
    return ctypes.addressof(a)


def u32(*vals):
    a = np.array(vals, dtype=np.uint32)
    _keep.append(a)
    return a.ctypes.data


F, F6, BAD = 0, 3, 99        # a 4-limb field, the 6-limb one, no id at all
C, C_BLS = 0, 2              # a curve with the endomorphism, the one without
BIG = 1 << 32                # a count one past what a call takes
N = None

CASES = [
    ("world_0", "plk_multi_plan", (0, 1, 16, 0, b, N, N, N)),
    ("device_beyond_world", "plk_multi_plan", (2, 1, 16, 2, b, N, N, N)),
    ("null_slots", "plk_multi_plan", (2, 1, 16, 0, N, N, N, N)),
    # ---- NTT ----
    ("bad_field", "plk_ntt_precompute_table", (BAD, 3, b)),
    ("log_n_31", "plk_ntt_precompute_table", (F, 31, b)),
    ("null_out", "plk_ntt_precompute_table", (F, 3, N)),
    ("bad_field", "plk_ntt_batch", (BAD, 3, 0, 2, ptrs(b, b), ptrs(b, b))),
    ("log_n_31", "plk_ntt_batch", (F, 31, 0, 2, ptrs(b, b), ptrs(b, b))),
    ("batch_0", "plk_ntt_batch", (F, 3, 0, 0, N, N)),
    ("null_in", "plk_ntt_batch", (F, 3, 0, 2, N, ptrs(b, b))),
    ("null_out", "plk_ntt_batch", (F, 3, 0, 2, ptrs(b, b), N)),
    ("null_in_slot_1", "plk_ntt_batch", (F, 3, 0, 2, ptrs(b, N), ptrs(b, b))),
    ("null_out_slot_0", "plk_ntt_batch", (F, 3, 0, 2, ptrs(b, b), ptrs(N, b))),
    ("bad_field", "plk_ntt", (BAD, 3, 0, b, b)),
    ("log_n_31", "plk_ntt", (F, 31, 0, b, b)),
    ("null_in", "plk_ntt", (F, 3, 0, N, b)),
    ("null_out", "plk_ntt", (F, 3, 0, b, N)),
    ("bad_field", "plk_ntt_padded_batch", (BAD, 3, 2, ptrs(b, b), sizes(4, 4), ptrs(b, b))),
    ("log_n_31", "plk_ntt_padded_batch", (F, 31, 2, ptrs(b, b), sizes(4, 4), ptrs(b, b))),
    ("batch_0", "plk_ntt_padded_batch", (F, 3, 0, N, N, N)),
    ("null_in", "plk_ntt_padded_batch", (F, 3, 2, N, sizes(4, 4), ptrs(b, b))),
    ("null_n_in", "plk_ntt_padded_batch", (F, 3, 2, ptrs(b, b), N, ptrs(b, b))),
    ("null_out", "plk_ntt_padded_batch", (F, 3, 2, ptrs(b, b), sizes(4, 4), N)),
    ("n_in_exceeds", "plk_ntt_padded_batch", (F, 3, 2, ptrs(b, b), sizes(4, 9), ptrs(b, b))),
    ("null_in_slot_1", "plk_ntt_padded_batch", (F, 3, 2, ptrs(b, N), sizes(4, 4), ptrs(b, b))),
    ("null_out_slot_1", "plk_ntt_padded_batch", (F, 3, 2, ptrs(b, b), sizes(4, 4), ptrs(b, N))),
    ("bad_field", "plk_ntt_padded", (BAD, 3, b, 4, b)),
    ("n_in_exceeds", "plk_ntt_padded", (F, 3, b, 9, b)),
    ("null_in", "plk_ntt_padded", (F, 3, N, 4, b)),
    ("null_out", "plk_ntt_padded", (F, 3, b, 4, N)),
    # ---- polynomials ----
    ("six_limb_field", "plk_poly_divide_by_z_h", (F6, b, 8, 4, b, 8, b)),
    ("null_out_len", "plk_poly_divide_by_z_h", (F, b, 8, 4, b, 8, N)),
    ("null_coeffs", "plk_poly_divide_by_z_h", (F, N, 8, 4, b, 8, b)),
    ("six_limb_field", "plk_poly_mul", (F6, b, 4, b, 4, b, 8, b)),
    ("null_out_len", "plk_poly_mul", (F, b, 4, b, 4, b, 8, N)),
    ("null_a", "plk_poly_mul", (F, N, 4, b, 4, b, 8, b)),
    ("null_b", "plk_poly_mul", (F, b, 4, N, 4, b, 8, b)),
    ("six_limb_field", "plk_poly_division", (F6, b, 8, b, 2, b, 7, N)),
    ("null_b", "plk_poly_division", (F, b, 8, N, 2, b, 7, N)),
    ("degree_0", "plk_poly_division", (F, b, 8, b, 1, b, 7, N)),
    ("degree_33", "plk_poly_division", (F, b, 64, b, 34, b, 64, N)),
    ("zero_lead", "plk_poly_division", (F, b, 8, z, 2, b, 7, N)),
    ("a_too_short", "plk_poly_division", (F, b, 1, b, 2, b, 7, N)),
    ("q_len_short", "plk_poly_division", (F, b, 8, b, 2, b, 6, N)),
    ("null_a", "plk_poly_division", (F, N, 8, b, 2, b, 7, N)),
    ("null_q", "plk_poly_division", (F, b, 8, b, 2, N, 7, N)),
    ("six_limb_field", "plk_poly_inv_mod_xn", (8, F6, b, 4, b)),
    ("n_0", "plk_poly_inv_mod_xn", (0, F, b, 4, b)),
    ("lh_0", "plk_poly_inv_mod_xn", (8, F, b, 0, b)),
    ("n_beyond_transform", "plk_poly_inv_mod_xn", (1 << 31, F, b, 4, b)),
    ("null_h", "plk_poly_inv_mod_xn", (8, F, N, 4, b)),
    ("null_out", "plk_poly_inv_mod_xn", (8, F, b, 4, N)),
    ("h0_zero", "plk_poly_inv_mod_xn", (8, F, z, 4, b)),
    ("six_limb_field", "plk_poly_div_rem", (8, F6, b, b, 2, b, 7, N)),
    ("degree_0", "plk_poly_div_rem", (8, F, b, b, 1, b, 7, N)),
    ("a_too_short", "plk_poly_div_rem", (1, F, b, b, 2, b, 7, N)),
    ("q_len_short", "plk_poly_div_rem", (8, F, b, b, 2, b, 6, N)),
    ("la_beyond_transform", "plk_poly_div_rem", (1 << 31, F, b, b, 2, b, 1 << 31, N)),
    ("null_a", "plk_poly_div_rem", (8, F, N, b, 2, b, 7, N)),
    ("null_b", "plk_poly_div_rem", (8, F, b, N, 2, b, 7, N)),
    ("null_q", "plk_poly_div_rem", (8, F, b, b, 2, N, 7, N)),
    ("zero_lead", "plk_poly_div_rem", (8, F, b, z, 2, b, 7, N)),
    # ---- the Plonk and Plookup provers ----
    ("six_limb_field", "plk_plonk_vanishing_points", (F6, 3, b, b, b, b, b, b, b, b, b, b, b)),
    ("log_degree_28", "plk_plonk_vanishing_points", (F, 28, b, b, b, b, b, b, b, b, b, b, b)),
    ("null_constants", "plk_plonk_vanishing_points", (F, 3, N, b, b, b, b, b, b, b, b, b, b)),
    ("null_out", "plk_plonk_vanishing_points", (F, 3, b, b, b, b, b, b, b, b, b, b, N)),
    ("six_limb_field", "plk_plonk_permutation_z_dev", (F6, 3, b, b, 1, b, b, b, b, b, N)),
    ("six_limb_field", "plk_plonk_permutation_z", (F6, 3, b, b, 1, b, b, b, b, N)),
    ("sigma_stride_2", "plk_plonk_permutation_z", (F, 3, b, b, 2, b, b, b, b, N)),
    ("log_degree_28", "plk_plonk_permutation_z", (F, 28, b, b, 1, b, b, b, b, N)),
    ("null_wires", "plk_plonk_permutation_z", (F, 3, N, b, 1, b, b, b, b, N)),
    ("null_out", "plk_plonk_permutation_z", (F, 3, b, b, 8, b, b, b, N, N)),
    ("six_limb_field", "plk_plookup_grand_product", (3, F6, b, b, b, b, b, b, N)),
    ("log_size_0", "plk_plookup_grand_product", (0, F, b, b, b, b, b, b, N)),
    ("log_size_29", "plk_plookup_grand_product", (29, F, b, b, b, b, b, b, N)),
    ("null_s", "plk_plookup_grand_product", (3, F, b, b, N, b, b, b, N)),
    ("six_limb_field", "plk_plookup_vanishing_points", (3, F6, b, b, b, b, b)),
    ("log_size_0", "plk_plookup_vanishing_points", (0, F, b, b, b, b, b)),
    ("log_size_29", "plk_plookup_vanishing_points", (29, F, b, b, b, b, b)),
    ("null_values", "plk_plookup_vanishing_points", (3, F, N, b, b, b, b)),
    ("log_size_0", "plk_plookup_sorted_multiset", (0, F, b, b, b, N)),
    ("log_size_29", "plk_plookup_sorted_multiset", (29, F, b, b, b, N)),
    ("six_limb_field", "plk_plookup_sorted_multiset", (3, F6, b, b, b, N)),
    ("null_t", "plk_plookup_sorted_multiset", (3, F, b, N, b, N)),
    ("six_limb_field", "plk_plonk_sigma", (3, F6, b, u32(0, 2), 1, b, b, N)),
    ("null_k_is", "plk_plonk_sigma", (3, F, b, u32(0, 2), 1, N, b, N)),
    ("log_degree_28", "plk_plonk_sigma", (28, F, b, u32(0, 2), 1, b, b, N)),
    ("too_many_partitions", "plk_plonk_sigma", (3, F, b, u32(0, 2), (1 << 31) + 1, b, b, N)),
    ("null_offsets", "plk_plonk_sigma", (3, F, b, N, 1, b, b, N)),
    ("no_output", "plk_plonk_sigma", (3, F, b, u32(0, 2), 1, b, N, N)),
    ("offsets_start_at_1", "plk_plonk_sigma", (3, F, b, u32(1, 2), 1, b, b, N)),
    ("offsets_decrease", "plk_plonk_sigma", (3, F, b, u32(0, 3, 2), 2, b, b, N)),
    ("too_many_members", "plk_plonk_sigma", (3, F, b, u32(0, 0x90000000), 1, b, b, N)),
    ("null_members", "plk_plonk_sigma", (3, F, N, u32(0, 2), 1, b, b, N)),
    ("six_limb_field", "plk_plonk_evaluate_all_constraints", (F6, 2, b, b, b, b, b, b, b)),
    ("count_0", "plk_plonk_evaluate_all_constraints", (F, 0, N, N, N, N, b, b, N)),
    ("null_below", "plk_plonk_evaluate_all_constraints", (F, 2, b, b, b, N, b, b, b)),
    # ---- the opening step ----
    ("null_x", "plk_field_powers_dev", (F, N, 4, b, N)),
    ("six_limb_field", "plk_field_powers", (F6, b, 4, b)),
    ("null_x", "plk_field_powers", (F, N, 4, b)),
    ("null_out", "plk_field_powers", (F, b, 4, N)),
    ("six_limb_field", "plk_plonk_eval_polys", (F6, 1, ptrs(b), sizes(4), 1, b, b)),
    ("n_points_0", "plk_plonk_eval_polys", (F, 1, ptrs(b), sizes(4), 0, b, b)),
    ("n_points_9", "plk_plonk_eval_polys", (F, 1, ptrs(b), sizes(4), 9, b, b)),
    ("null_points", "plk_plonk_eval_polys", (F, 1, ptrs(b), sizes(4), 1, N, b)),
    ("null_lens", "plk_plonk_eval_polys", (F, 1, ptrs(b), N, 1, b, b)),
    ("six_limb_field", "plk_poly_reduce", (F6, 1, ptrs(b), sizes(4), b, 4, b)),
    ("null_scalars", "plk_poly_reduce", (F, 1, ptrs(b), sizes(4), N, 4, b)),
    ("null_out", "plk_poly_reduce", (F, 1, ptrs(b), sizes(4), b, 4, N)),
    ("longer_than_degree", "plk_poly_reduce", (F, 2, ptrs(b, b), sizes(4, 5), b, 4, b)),
    ("six_limb_field", "plk_halo_build_b", (F6, 1, b, b, 4, b)),
    ("n_points_0", "plk_halo_build_b", (F, 0, b, b, 4, b)),
    ("n_points_9", "plk_halo_build_b", (F, 9, b, b, 4, b)),
    ("null_v", "plk_halo_build_b", (F, 1, b, N, 4, b)),
    ("null_out", "plk_halo_build_b", (F, 1, b, b, 4, N)),
    ("six_limb_field", "plk_halo_s", (F6, 2, b, b)),
    ("k_31", "plk_halo_s", (F, 31, b, b)),
    ("null_us", "plk_halo_s", (F, 2, N, b)),
    ("null_out", "plk_halo_s", (F, 2, b, N)),
    ("zero_challenge", "plk_halo_s", (F, 2, z, b)),
    # ---- MSM ----
    ("bad_curve", "plk_msm_precompute_ex", (BAD, 16, b, N, 0, 0, b)),
    ("null_bases", "plk_msm_precompute_ex", (C, 16, N, N, 0, 0, b)),
    ("bad_curve", "plk_msm_precompute", (BAD, 16, b, N, 0, b)),
    ("null_bases", "plk_msm_precompute", (C, 16, N, N, 0, b)),
    ("null_context", "plk_msm_free", (N,)),
    ("null_context", "plk_msm_execute_projective_dev", (N, 1, b, 16, b, b, N)),
    ("null_context", "plk_msm_execute_projective", (N, b, 16, b, b)),
    ("null_bucket_parts", "plk_msm_execute_parts_buckets_dev", (N, 1, b, b, b, N, N, b, b, N)),
    ("null_context", "plk_msm_execute_batch", (N, 1, ptrs(b), 16, b, b)),
    ("null_context", "plk_msm_execute", (N, b, 16, b, b)),
    ("bad_curve", "plk_msm", (BAD, 16, b, N, b, b, b)),
    ("null_bases", "plk_msm", (C, 16, N, N, b, b, b)),
    ("bad_curve", "plk_curve_sum_affine", (BAD, 4, b, N, b, b)),
    ("null_points", "plk_curve_sum_affine", (C, 4, N, N, b, b)),
    ("null_out_zero", "plk_curve_sum_affine", (C, 4, b, N, b, N)),
    ("bad_curve", "plk_msm_table_digits", (BAD, 8)),
    ("window_0", "plk_msm_table_digits", (C, 0)),
    ("bad_curve", "plk_msm_precompute_table", (BAD, 4, b, N, 8, b, b)),
    ("window_0", "plk_msm_precompute_table", (C, 4, b, N, 0, b, b)),
    ("window_65", "plk_msm_precompute_table", (C, 4, b, N, 65, b, b)),
    ("null_out_zero", "plk_msm_precompute_table", (C, 4, b, N, 8, b, N)),
    ("n_0", "plk_msm_precompute_table", (C, 0, N, N, 8, N, N)),
    ("bad_curve", "plk_curve_fold_pairs", (BAD, 4, b, N, b, N, b, b, b, b)),
    ("null_hi", "plk_curve_fold_pairs", (C, 4, b, N, N, N, b, b, b, b)),
    ("null_scalar", "plk_curve_fold_pairs", (C, 4, b, N, b, N, b, N, b, b)),
    ("m_0", "plk_curve_fold_pairs", (C, 0, N, N, N, N, b, b, N, N)),
    # ---- inversion, normalisation, byte encodings ----
    ("bad_field", "plk_field_batch_inverse_dev", (BAD, b, b, b, 4, N)),
    ("bad_field", "plk_field_batch_inverse", (BAD, b, b, 4)),
    ("count_0", "plk_field_batch_inverse", (F, N, N, 0)),
    ("null_out", "plk_field_batch_inverse", (F, b, N, 4)),
    ("null_is_none", "plk_field_batch_inverse_opt", (F, b, b, N, 4)),
    ("bad_field", "plk_field_batch_inverse_opt", (BAD, b, b, b, 4)),
    ("count_0", "plk_field_batch_inverse_opt", (F, N, N, N, 0)),
    ("null_x", "plk_field_batch_inverse_opt", (F, N, b, b, 4)),
    ("bad_curve", "plk_curve_batch_to_affine", (BAD, 4, b, N, b, b)),
    ("count_0", "plk_curve_batch_to_affine", (C, 0, N, N, N, N)),
    ("null_out_xy", "plk_curve_batch_to_affine", (C, 4, b, N, N, b)),
    ("bad_field", "plk_field_to_bytes", (BAD, b, 4, b)),
    ("count_0", "plk_field_to_bytes", (F, N, 0, N)),
    ("null_x", "plk_field_to_bytes", (F, N, 4, b)),
    ("bad_field", "plk_field_from_bytes", (BAD, b, 4, b)),
    ("count_0", "plk_field_from_bytes", (F, N, 0, N)),
    ("null_out", "plk_field_from_bytes", (F, b, 4, N)),
    ("bad_curve", "plk_curve_point_to_bytes", (BAD, b, N, 4, b)),
    ("count_0", "plk_curve_point_to_bytes", (C, N, N, 0, N)),
    ("null_out", "plk_curve_point_to_bytes", (C, b, N, 4, N)),
    ("bad_curve", "plk_curve_point_from_bytes", (BAD, b, 4, b, b, N)),
    ("count_0", "plk_curve_point_from_bytes", (C, N, 0, N, N, N)),
    ("null_out_zero", "plk_curve_point_from_bytes", (C, b, 4, b, N, N)),
    # ---- hashes to the curve, Rescue ----
    ("bad_curve", "plk_hash_to_curve", (4, BAD, 0, b)),
    ("count_2^32", "plk_hash_to_curve", (BIG, C, 0, b)),
    ("count_0", "plk_hash_to_curve", (0, C, 0, N)),
    ("null_out", "plk_hash_to_curve", (4, C, 0, N)),
    ("bad_curve", "plk_hash_field_to_curve", (4, BAD, b, b)),
    ("count_2^32", "plk_hash_field_to_curve", (BIG, C, b, b)),
    ("count_0", "plk_hash_field_to_curve", (0, C, N, N)),
    ("null_seeds", "plk_hash_field_to_curve", (4, C, N, b)),
    ("bad_field", "plk_blake_field", (4, BAD, b, b, b, b)),
    ("count_2^32", "plk_blake_field", (BIG, F, b, b, b, b)),
    ("count_0", "plk_blake_field", (0, F, N, N, N, N)),
    ("null_iters", "plk_blake_field", (4, F, N, b, b, b)),
    ("bad_field", "plk_rescue_mds", (4, BAD, b)),
    ("width_3", "plk_rescue_mds", (3, F, b)),
    ("null_out", "plk_rescue_mds", (4, F, N)),
    ("null_context", "plk_rescue_permutation", (4, N, b, b)),
    ("null_context", "plk_rescue_sponge", (4, N, 2, b, 1, b)),
    ("null_context", "plk_rescue_hash_to_curve", (4, N, C, 0, b)),
    ("null_context", "plk_rescue_hash_field_to_curve", (4, N, C, b, b)),
    ("bad_field", "plk_field_kth_root", (4, BAD, 5, b, b)),
    ("k_0", "plk_field_kth_root", (4, F, 0, b, b)),
    ("k_2_no_permutation", "plk_field_kth_root", (4, F, 2, b, b)),
    ("count_2^32", "plk_field_kth_root", (BIG, F, 5, b, b)),
    ("count_0", "plk_field_kth_root", (0, F, 5, N, N)),
    ("null_in", "plk_field_kth_root", (4, F, 5, N, b)),
    # ---- a point times a scalar, the Halo endomorphism ----
    ("bad_curve", "plk_curve_scalar_mul", (4, BAD, 4, b, 4, b, N, b, b)),
    ("count_2^32", "plk_curve_scalar_mul", (BIG, C, 1, b, 1, b, N, b, b)),
    ("count_0", "plk_curve_scalar_mul", (0, C, 0, N, 0, N, N, N, N)),
    ("n_scalars_3_of_4", "plk_curve_scalar_mul", (4, C, 3, b, 4, b, N, b, b)),
    ("null_out_zero", "plk_curve_scalar_mul", (4, C, 4, b, 4, b, N, b, N)),
    ("bad_curve", "plk_halo_n_mul", (4, BAD, 128, 4, b, 4, b, N, b, b)),
    ("no_endomorphism", "plk_halo_n_mul", (4, C_BLS, 128, 4, b, 4, b, N, b, b)),
    ("security_bits_0", "plk_halo_n_mul", (4, C, 0, 4, b, 4, b, N, b, b)),
    ("n_points_3_of_4", "plk_halo_n_mul", (4, C, 128, 4, b, 3, b, N, b, b)),
    ("count_0", "plk_halo_n_mul", (0, C, 128, 0, N, 0, N, N, N, N)),
    ("null_scalars", "plk_halo_n_mul", (4, C, 128, 4, N, 4, b, N, b, b)),
    ("bad_curve", "plk_halo_n", (4, BAD, 128, b, b)),
    ("no_endomorphism", "plk_halo_n", (4, C_BLS, 128, b, b)),
    ("security_bits_odd", "plk_halo_n", (4, C, 127, b, b)),
    ("security_bits_1024", "plk_halo_n", (4, C, 1024, b, b)),
    ("count_2^32", "plk_halo_n", (BIG, C, 128, b, b)),
    ("count_0", "plk_halo_n", (0, C, 128, N, N)),
    ("null_out", "plk_halo_n", (4, C, 128, b, N)),
    # ---- the inner-product argument ----
    ("null_tables", "plk_halo_begin_tabled_dev", (C, 16, b, b, b, N, N, b, b, 0, 0, N, 0, 0, N, b)),
    ("bad_curve", "plk_halo_begin", (BAD, 16, b, b, b, N, b, b, 0, b)),
    ("null_b", "plk_halo_begin", (C, 16, b, N, b, N, b, b, 0, b)),
    ("null_context", "plk_halo_free", (N,)),
    # ---- self-test, checked build, utilities ----
    ("bad_curve", "plk_selftest_quad", (BAD, b, 64, 4, b)),
    ("null_points", "plk_selftest_quad", (C, N, 64, 4, b)),
    ("n_0", "plk_selftest_quad", (C, b, 0, 4, b)),
    ("null_counts", "plk_checked_failures", (N,)),
    ("bad_curve", "plk_msm_debug_digits", (BAD, 8, 4, b, b, b)),
    ("digit_count_only", "plk_msm_debug_digits", (C, 8, 4, b, N, w)),
    ("null_scalars", "plk_msm_debug_digits", (C, 8, 4, N, b, w)),
    ("bad_curve", "plk_curve_op", (BAD, 0, 0, 4, b, N, b, b, N, b, b, b, b, w)),
    ("op_9", "plk_curve_op", (C, 9, 0, 4, b, N, b, b, N, b, b, b, b, w)),
    ("count_2049", "plk_curve_op", (C, 0, 0, 2049, b, N, b, b, N, b, b, b, b, w)),
    ("doublings_0", "plk_curve_op", (C, 6, 0, 4, b, N, b, b, N, b, b, b, b, w)),
    ("groups_of_3", "plk_curve_op", (C, 7, 3, 4, b, N, b, b, N, b, b, b, b, w)),
    ("null_mismatch", "plk_curve_op", (C, 0, 0, 4, b, N, b, b, N, b, b, b, b, N)),
    ("count_0", "plk_curve_op", (C, 0, 0, 0, N, N, N, N, N, N, N, N, N, w)),
    ("null_b_lambda", "plk_curve_op", (C, 0, 0, 4, b, N, b, b, N, N, b, b, b, w)),
    ("bad_curve", "plk_curve_gen_bases_dev", (BAD, 4, 0, b, b, b, N)),
    ("null_d", "plk_curve_gen_bases_dev", (C, 4, 0, b, N, b, N)),
]

# every other entry of lib.SYMBOLS, and why it has no case
_FORWARDER = "forwards to an implementation in another unit: the wrapper has no check of its own"
_CONTEXT = "its first check reads a live context, which needs a device to build"
_NO_REFUSAL = "no refusal: reads or sets process state"
EXCLUDED = {name: _FORWARDER for name in """plk_ntt_precompute_table_dev plk_ntt_dev plk_ntt_padded_dev plk_poly_divide_by_z_h_dev plk_poly_mul_dev
    plk_poly_division_dev plk_poly_inv_mod_xn_dev plk_poly_div_rem_dev plk_plonk_vanishing_points_dev plk_plookup_grand_product_dev
    plk_plookup_vanishing_points_dev plk_plookup_sorted_multiset_dev plk_plonk_sigma_dev plk_plonk_eval_polys_dev plk_poly_reduce_dev
    plk_halo_build_b_dev plk_halo_s_dev plk_msm_precompute_dev plk_msm_precompute_dev_ex plk_msm_execute_dev plk_msm_execute_parts_dev
    plk_msm_combine_partials_dev plk_msm_precompute_table_dev plk_curve_fold_pairs_dev plk_curve_batch_to_affine_dev plk_hash_to_curve_dev
    plk_hash_field_to_curve_dev plk_rescue_permutation_dev plk_rescue_sponge_dev plk_field_kth_root_dev plk_rescue_hash_to_curve_dev
    plk_rescue_hash_field_to_curve_dev plk_curve_scalar_mul_dev plk_halo_n_dev plk_halo_n_mul_dev plk_field_inner_product_dev
    plk_field_fold_slices_dev plk_halo_begin_dev plk_curve_fold_multi_dev plk_ntt_precompute plk_poly_from_roots plk_field_op
    plk_bench_ceilings plk_rescue_create plk_rescue_free plk_rescue_rounds""".split()}
EXCLUDED.update({name: _CONTEXT for name in """plk_msm_ctx_len plk_msm_ctx_window plk_halo_round_lr plk_halo_round_fold plk_halo_len
    plk_halo_frozen plk_halo_read plk_msm_set_profiling plk_msm_get_timings""".split()})
EXCLUDED.update({name: _NO_REFUSAL for name in """plk_init plk_init_devices plk_device_count plk_group_copy_stats plk_thread_hip_device
    plk_shutdown plk_last_error plk_min_gpu_log_n plk_field_limbs plk_curve_limbs plk_curve_scalar_field plk_ntt_clear_cache
    plk_msm_partials_bytes plk_checked_build plk_ntt_set_profiling plk_ntt_get_timings""".split()})
EXCLUDED["plk_set_thread_device"] = "its refusal text names the size of the device group, which other tests of a session change"
# Not reachable without a live context, so not listed above either: the length mismatch of plk_msm_execute* (the null-context
# check comes first and the length is read from the context), and the checks of the Rescue entries behind the context's field.


def case_id(label, entry):
    return "%s:%s" % (entry, label)


def run(L):
    """{case id: [code, text]}; the text only of a refusal (a PLK_OK return leaves an earlier call's text in place)"""
    got = {}
    for label, entry, args in CASES:
        rc = getattr(L, entry)(*args)
        got[case_id(label, entry)] = [rc, L.plk_last_error().decode() if rc else None]
    return got


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from plonky_amd import lib
    with open(sys.argv[1], "w") as fh:
        json.dump(run(lib.load()), fh, indent=0, sort_keys=True)
        fh.write("\n")
