"""The BLAKE3 hash to the curve on the device (plonky_amd/csrc/hash_to_curve.hip) against tests/hash_to_curve_ref.py, limb for limb:
blake_field on all six fields, the integer and the field-element entries on all five curves at the wave edges and beyond one
workgroup, ranges against their parts, the device forms on a stream of their own, the loop form behind PLK_H2C_NAIVE, the checked
build, the refusals, and the generators of a 2^10 circuit through an MSM context.  The Python reference is the slow side (about a
millisecond per seed); its results are cached per (curve, seed) and shared by the tests."""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle import bigint_ref as br
from plonky_amd import api, lib, synth
from tests import checked_child
from tests import hash_to_curve_ref as h2c

pytestmark = pytest.mark.gpu

CURVES = sorted(br.CURVES)
COUNTS = (1, 63, 64, 65, 257, 1000)         # the edges of a wave, more than one workgroup, a size that is no multiple of anything
STARTS = (0, 5, (1 << 32) + 7)              # the last: a non-zero high word, canonical bytes above the fourth


def ref_range(curve, start, count):
    return h2c.points_mont(curve, range(start, start + count))


def on_curve(curve, pts):
    c = br.CURVES[curve]
    f = c.base.field_id
    for k, (x, y) in enumerate(pts):
        xi, yi = synth.from_mont(f, x), synth.from_mont(f, y)
        assert (yi * yi - xi * xi * xi - c.b) % c.base.p == 0, k


@pytest.mark.parametrize("field", sorted(br.FIELDS))
def test_blake_field_matches_the_reference(field):
    f = br.FIELDS[field]
    edge = [0, 1, f.p - 1, (1 << 64) - 1, (1 << 128) - 1, (1 << 192) - 1, (1 << (f.bits - 1)) - 1]
    rand = [synth.from_mont(field, r) for r in synth.rand_field(field, 0xB1A4E, 200 - len(edge))]
    seeds = edge + rand
    iters = np.array([(0, 1, 2, 3, 7, 128, 254, 255)[k % 8] for k in range(len(seeds))], dtype=np.uint8)
    x, y_neg = api.blake_field(field, iters, np.stack([synth.mont(field, s) for s in seeds]))
    js = 0
    for k, s in enumerate(seeds):
        ex, ey, j = h2c.blake_field(field, int(iters[k]), s)
        assert synth.from_mont(field, x[k]) == ex and int(y_neg[k]) == ey, (k, s)
        js += j > 0
    assert js > 0 and set(y_neg.tolist()) == {0, 1}


@pytest.mark.parametrize("curve", CURVES)
def test_usize_entry_matches_the_reference_limb_for_limb(curve):
    for start in STARTS:
        exp = ref_range(curve, start, max(COUNTS))
        for count in COUNTS:
            got = api.blake_hash_usize_to_curve(curve, start, count)
            assert got.shape == exp[:count].shape and np.array_equal(got, exp[:count]), (start, count)
    assert np.array_equal(api.blake_hash_usize_to_curve(curve, 5), exp_single(curve, 5))


def exp_single(curve, seed):
    return ref_range(curve, seed, 1)[0]


def test_two_thousand_seeds_shrink_the_work_list_below_a_wave():
    """2^11 seeds on Tweedledee: 14 rounds, the list falls below one workgroup and below one wave on the way"""
    got = api.blake_hash_usize_to_curve(api.TWEEDLEDEE, 0, 1 << 11)
    assert np.array_equal(got, ref_range(api.TWEEDLEDEE, 0, 1 << 11))
    tries = [h2c.hash_usize_to_curve(api.TWEEDLEDEE, s)[2] for s in range(1 << 11)]
    assert max(tries) >= 7  # the list was still not empty after seven rounds


@pytest.mark.parametrize("curve", CURVES)
def test_a_range_is_the_concatenation_of_its_parts(curve):
    a, n = 3, 700
    whole = api.blake_hash_usize_to_curve(curve, a, n)
    for m in (1, 64, 333):
        parts = np.concatenate([api.blake_hash_usize_to_curve(curve, a, m), api.blake_hash_usize_to_curve(curve, a + m, n - m)])
        assert np.array_equal(whole, parts), m


def test_sixty_five_thousand_seeds_sampled_split_and_on_the_curve():
    curve, a, n = api.TWEEDLEDEE, 11, 1 << 16
    whole = api.blake_hash_usize_to_curve(curve, a, n)
    rng = np.random.default_rng(0x2C16)
    sample = sorted(set([0, 63, 64, n - 1] + rng.integers(0, n, 252).tolist()))
    assert np.array_equal(whole[sample], h2c.points_mont(curve, [a + k for k in sample]))
    on_curve(curve, whole)
    m = 21845
    parts = np.concatenate([api.blake_hash_usize_to_curve(curve, a, m), api.blake_hash_usize_to_curve(curve, a + m, n - m)])
    assert np.array_equal(whole, parts)


@pytest.mark.parametrize("curve", CURVES)
def test_field_entry_agrees_with_the_usize_entry_and_the_reference(curve):
    f = br.CURVES[curve].base.field_id
    ks = list(range(130)) + [(1 << 32) + 7, (1 << 64) - 1]
    seeds = np.stack([synth.mont(f, k) for k in ks])
    got = api.blake_hash_base_field_to_curve(curve, seeds)
    assert np.array_equal(got[:130], api.blake_hash_usize_to_curve(curve, 0, 130))
    assert np.array_equal(got[130], api.blake_hash_usize_to_curve(curve, (1 << 32) + 7))
    assert np.array_equal(got[131], api.blake_hash_usize_to_curve(curve, (1 << 64) - 1))
    rand = synth.rand_field(f, 0x5EED + curve, 200)  # the shape of test_hash_blake_deterministic (hash_to_curve.rs:133)
    got = api.blake_hash_base_field_to_curve(curve, rand)
    assert np.array_equal(got, h2c.points_mont(curve, [synth.from_mont(f, r) for r in rand]))
    assert np.array_equal(got, api.blake_hash_base_field_to_curve(curve, rand))  # two calls, the same bytes


def test_device_forms_on_a_stream_of_their_own_equal_the_host_forms():
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    side = torch.cuda.Stream()
    for curve in (api.TWEEDLEDEE, api.BLS12_377):
        f = br.CURVES[curve].base.field_id
        rand = synth.rand_field(f, 0xD5 + curve, 300)
        with torch.cuda.stream(side):
            a = dev.hash_to_curve_dev(curve, 1000, seed_start=5)
            b = dev.hash_to_curve_dev(curve, 300, seeds=dev.to_device(rand))
            a2 = dev.hash_to_curve_dev(curve, 1000, seed_start=5)
        side.synchronize()
        assert np.array_equal(dev.to_host(a), api.blake_hash_usize_to_curve(curve, 5, 1000))
        assert np.array_equal(dev.to_host(b), api.blake_hash_base_field_to_curve(curve, rand))
        assert dev.to_host(a).tobytes() == dev.to_host(a2).tobytes()


CHILD = r'''
import hashlib, sys
import numpy as np
from plonky_amd import api, synth
h = hashlib.sha256()
for curve, start, count in ((0, 0, 1), (0, 5, 65), (0, (1 << 32) + 7, 257), (0, 0, 2048), (2, 0, 257), (1, 5, 64), (3, 0, 63), (4, 0, 1000)):
    h.update(api.blake_hash_usize_to_curve(curve, start, count).tobytes())
h.update(api.blake_hash_base_field_to_curve(2, synth.rand_field(3, 77, 200)).tobytes())
x, y_neg = api.blake_field(3, 2, synth.rand_field(3, 78, 100))
h.update(x.tobytes() + y_neg.tobytes())
print("DIGEST", h.hexdigest())
'''


def small_set_digest():
    h = hashlib.sha256()
    for curve, start, count in ((0, 0, 1), (0, 5, 65), (0, (1 << 32) + 7, 257), (0, 0, 2048), (2, 0, 257), (1, 5, 64), (3, 0, 63), (4, 0, 1000)):
        h.update(ref_range(curve, start, count).tobytes())
    rand = synth.rand_field(3, 77, 200)
    h.update(h2c.points_mont(2, [synth.from_mont(3, r) for r in rand]).tobytes())
    xs, ys = [], []
    for r in synth.rand_field(3, 78, 100):
        x, y_neg, _ = h2c.blake_field(3, 2, synth.from_mont(3, r))
        xs.append(synth.mont(3, x))
        ys.append(y_neg)
    h.update(np.stack(xs).tobytes() + np.array(ys, dtype=np.uint8).tobytes())
    return h.hexdigest()


def test_the_loop_form_behind_the_knob_gives_the_same_bytes():
    """knobs are read once: the loop form runs in a process of its own"""
    assert "DIGEST " + small_set_digest() in checked_child.run_child(CHILD, PLK_H2C_NAIVE="1")


def test_the_small_set_through_the_checked_build():
    assert "DIGEST " + small_set_digest() in checked_child.run_checked(CHILD)


def test_generators_of_a_circuit_commit_like_the_reference_generators():
    """pedersen_generators(Tweedledee, 2^10) in an MSM context: a commitment equals plk_msm over the reference's generators"""
    curve, degree = api.TWEEDLEDEE, 1 << 10
    g, h, u = api.pedersen_generators(curve, degree)
    exp = ref_range(curve, 0, degree + 2)
    assert np.array_equal(h, exp[degree]) and np.array_equal(u, exp[degree + 1])
    scalars = synth.rand_field(api.CURVE_SCALAR_FIELD[curve], 0xC0117, degree)
    pre = api.msm_precompute(curve, g, 8)
    got, gz = api.msm_execute_parallel(pre, scalars)
    want, wz = api.msm_parallel(curve, scalars, exp[:degree], 8)
    assert gz == wz == 0 and np.array_equal(got, want)
    # and from device memory, as plk_hash_to_curve_dev leaves them
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    dpre = dev.msm_precompute_dev(curve, dev.hash_to_curve_dev(curve, degree))
    oxy, oz = dev.msm_execute_dev(dpre, dev.to_device(scalars))
    torch.cuda.synchronize()
    assert int(oz.cpu()[0]) == 0 and np.array_equal(dev.to_host(oxy).reshape(2, -1), want)


def test_refusals_launch_nothing_and_return_the_documented_codes():
    L = lib.load()
    buf = np.zeros((4, 2, 6), dtype=np.uint64)
    seeds = np.zeros((4, 6), dtype=np.uint64)
    iters = np.zeros(4, dtype=np.uint8)
    y_neg = np.zeros(4, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    d = torch.zeros((4, 2, 6), dtype=torch.int64, device="cuda")
    dp = ctypes.c_void_p(d.data_ptr())
    for bad in (-1, 5, 99):  # curve ids are 0..4
        assert L.plk_hash_to_curve(4, bad, 0, p(buf)) == lib.PLK_ERR_INVALID_ARG and b"bad curve id" in L.plk_last_error()
        assert L.plk_hash_to_curve_dev(4, bad, 0, dp, None) == lib.PLK_ERR_INVALID_ARG
        assert L.plk_hash_field_to_curve(4, bad, p(seeds), p(buf)) == lib.PLK_ERR_INVALID_ARG
        assert L.plk_hash_field_to_curve_dev(4, bad, dp, dp, None) == lib.PLK_ERR_INVALID_ARG
        assert L.plk_hash_to_curve(0, bad, 0, p(buf)) == lib.PLK_ERR_INVALID_ARG  # the id is checked before the count
    for bad in (-1, 6, 99):  # field ids are 0..5
        assert L.plk_blake_field(4, bad, p(iters), p(seeds), p(buf), p(y_neg)) == lib.PLK_ERR_INVALID_ARG and b"bad field id" in L.plk_last_error()
    # null pointers
    assert L.plk_hash_to_curve(4, 0, 0, None) == lib.PLK_ERR_INVALID_ARG
    assert L.plk_hash_to_curve_dev(4, 0, 0, None, None) == lib.PLK_ERR_INVALID_ARG
    assert L.plk_hash_field_to_curve(4, 0, None, p(buf)) == lib.PLK_ERR_INVALID_ARG
    assert L.plk_hash_field_to_curve(4, 0, p(seeds), None) == lib.PLK_ERR_INVALID_ARG
    assert L.plk_hash_field_to_curve_dev(4, 0, None, dp, None) == lib.PLK_ERR_INVALID_ARG
    assert L.plk_hash_field_to_curve_dev(4, 0, dp, None, None) == lib.PLK_ERR_INVALID_ARG
    for args in ((None, p(seeds), p(buf), p(y_neg)), (p(iters), None, p(buf), p(y_neg)), (p(iters), p(seeds), None, p(y_neg)),
                 (p(iters), p(seeds), p(buf), None)):
        assert L.plk_blake_field(4, 0, *args) == lib.PLK_ERR_INVALID_ARG
    # count == 0: PLK_OK, nothing read or written (null pointers pass)
    assert L.plk_hash_to_curve(0, 0, 0, None) == lib.PLK_OK
    assert L.plk_hash_to_curve_dev(0, 0, 0, None, None) == lib.PLK_OK
    assert L.plk_hash_field_to_curve(0, 0, None, None) == lib.PLK_OK
    assert L.plk_hash_field_to_curve_dev(0, 0, None, None, None) == lib.PLK_OK
    assert L.plk_blake_field(0, 0, None, None, None, None) == lib.PLK_OK
    torch.cuda.synchronize()
    assert not d.any().item() and not buf.any()
    assert api.blake_hash_usize_to_curve(0, 0, 0).shape == (0, 2, 4)
