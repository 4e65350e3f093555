"""The Rescue hash to the curve on the device (plonky_amd/csrc/rescue_h2c.hip) against tests/rescue_h2c_ref.py, limb for limb: all five
curves at 16 rounds at the edges of a quad, of a wave's 16 quads and of a workgroup; a work list compacted over many waves; seeds chosen
by the number of tries they take (the last round, the first and a later try of the closing launch); both forms of seed; the loop form
behind PLK_H2C_NAIVE; the checked build; the refusals; and the points through an MSM context.

The Python reference is the slow side (a few milliseconds per try at 16 rounds), so everything beyond the edge counts runs on a
1-round context: the round loop is the permutation's own (tests/test_gpu_rescue.py), what is walked here is the tries."""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle import bigint_ref as br
from plonky_amd import api, lib, synth
from tests import checked_child
from tests import rescue_h2c_ref as ref
from tests import rescue_ref as rr

pytestmark = pytest.mark.gpu

CURVES = sorted(br.CURVES)
COUNTS = (1, 2, 15, 16, 17, 63, 64, 65, 257)  # a quad is a seed, a wave 16 seeds, a workgroup one wave
DEE = api.TWEEDLEDEE


def make_ctx(curve, rounds, seed=1337):
    field = br.CURVES[curve].base.field_id
    consts = rr.constants(field, 4, rounds, seed)
    limbs = np.array(rr.constants_limbs(field, consts), dtype=np.uint64).reshape(rounds, 2, 4, -1)
    return api.RescueContext(field, limbs), consts


def ref_points(curve, rounds, consts, seeds):
    return ref.points_mont(curve, seeds, consts, key=(rounds, 1337))


def mont_seeds(curve, seeds):
    f = br.CURVES[curve].base.field_id
    return np.stack([synth.mont(f, s) for s in seeds])


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    return torch, dev


@pytest.fixture(scope="module")
def dee1():
    """Tweedledee with a 1-round context, and the tries of the integer seeds 0 .. 2^12 - 1"""
    ctx, consts = make_ctx(DEE, 1)
    exp, tries = ref_points(DEE, 1, consts, range(1 << 12))
    yield ctx, consts, exp, tries
    ctx.free()


PERIOD = 67  # shares no factor with a quad, a wave or a workgroup: every lane position still meets every seed of the pool


@pytest.mark.parametrize("curve", CURVES)
def test_all_curves_at_the_edges_of_a_quad_a_wave_and_a_workgroup(curve):
    """The reference costs 5 to 20 ms per try at 16 rounds, so the seeds of a batch repeat with a period that shares no factor with the
    quad, the wave or the workgroup; a wrong index still lands on another seed's point.  The pool is computed once per curve."""
    ctx, consts = make_ctx(curve, 16)
    with ctx:
        exp, tries = ref_points(curve, 16, consts, range(PERIOD))
        assert max(tries) >= 3
        pool = mont_seeds(curve, range(PERIOD))
        for count in COUNTS:
            idx = [(i + count) % PERIOD for i in range(count)]
            got = api.hash_base_field_to_curve(ctx, curve, pool[idx])
            assert got.shape == exp[idx].shape and np.array_equal(got, exp[idx]), (count, np.argwhere(got != exp[idx])[:4].tolist())
        for count in (1, 17, PERIOD):  # the integer form over the same seeds
            assert np.array_equal(api.hash_usize_to_curve(ctx, curve, 0, count), exp[:count]), count
        assert np.array_equal(api.hash_usize_to_curve(ctx, curve, 5), exp[5]) and np.array_equal(api.hash_u32_to_curve(ctx, curve, 5), exp[5])
        assert api.hash_usize_to_curve(ctx, curve, 0, 0).shape == (0, 2, exp.shape[2])  # count 0: nothing launched


def test_a_work_list_compacted_over_many_waves(dee1):
    """2^12 seeds are 256 waves in round 0 and 14 rounds: the list falls below a wave and below a quad on the way.  All are compared."""
    ctx, consts, exp, tries = dee1
    got = api.hash_usize_to_curve(ctx, DEE, 0, 1 << 12)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:4].tolist()
    assert max(tries) >= 7 and 0.4 < sum(t == 0 for t in tries) / len(tries) < 0.6


def test_seeds_chosen_by_their_tries_at_count_one(dee1):
    """count 1 is 3 rounds (tries 0, 1, 2), then the closing launch from try 3"""
    ctx, consts, exp, tries = dee1
    for want in (0, 2, 3, 5):  # no round needed, the last round, the first try of the tail, two tries into the tail
        seed = tries.index(want)
        got = api.hash_usize_to_curve(ctx, DEE, seed, 1)
        assert np.array_equal(got[0], exp[seed]), (want, seed)
        assert np.array_equal(api.hash_base_field_to_curve(ctx, DEE, synth.mont(0, seed)), exp[seed]), (want, seed)


def test_a_batch_whose_every_seed_needs_two_tries_or_more_and_both_signs(dee1):
    ctx, consts, exp, tries = dee1
    late = [s for s in range(1 << 12) if tries[s] >= 2][:200]
    assert len(late) == 200
    got = api.hash_base_field_to_curve(ctx, DEE, mont_seeds(DEE, late))
    assert np.array_equal(got, exp[late])
    batch = list(range(64))
    signs = {ref.try_outputs(DEE, s, tries[s], consts)[1] for s in batch}
    assert signs == {0, 1}  # the reference's side: both values of y_neg occur in this batch
    assert np.array_equal(api.hash_base_field_to_curve(ctx, DEE, mont_seeds(DEE, batch)), exp[batch])


@pytest.mark.parametrize("curve", (DEE, api.BLS12_377))
def test_field_seeds_integer_seeds_and_their_agreement(curve):
    f = br.CURVES[curve].base
    ctx, consts = make_ctx(curve, 1)
    with ctx:
        rnd = [synth.from_mont(f.field_id, r) for r in synth.rand_field(f.field_id, 0x5EED + curve, 20)]
        seeds = [0, 1, f.p - 1] + rnd
        exp, _ = ref_points(curve, 1, consts, seeds)
        assert np.array_equal(api.hash_base_field_to_curve(ctx, curve, mont_seeds(curve, seeds)), exp)
        for start, count in ((0, 3), ((1 << 32) - 1, 3), (1 << 32, 2), ((1 << 64) - 1, 1)):
            ints = [start + k for k in range(count)]
            e, _ = ref_points(curve, 1, consts, ints)
            got = api.hash_usize_to_curve(ctx, curve, start, count)
            assert np.array_equal(got, e), start
            assert np.array_equal(api.hash_base_field_to_curve(ctx, curve, mont_seeds(curve, ints)), got), start  # the two forms agree
        assert np.array_equal(api.hash_u32_to_curve(ctx, curve, (1 << 32) - 1), ref_points(curve, 1, consts, [(1 << 32) - 1])[0][0])
        a = api.hash_usize_to_curve(ctx, curve, 7, 130)
        assert np.array_equal(a, api.hash_base_field_to_curve(ctx, curve, mont_seeds(curve, range(7, 137))))


def test_two_runs_and_the_host_and_device_forms_give_the_same_bytes(dee1, torch_dev):
    torch, dev = torch_dev
    ctx, consts, exp, tries = dee1
    n = 1000
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = dev.rescue_hash_to_curve_dev(ctx, DEE, n, seed_start=5)
        a2 = dev.rescue_hash_to_curve_dev(ctx, DEE, n, seed_start=5)
        b = dev.rescue_hash_field_to_curve_dev(ctx, DEE, dev.to_device(mont_seeds(DEE, range(5, 5 + n))))
    side.synchronize()
    host = api.hash_usize_to_curve(ctx, DEE, 5, n)
    assert np.array_equal(host, exp[5:5 + n])
    assert dev.to_host(a).tobytes() == dev.to_host(a2).tobytes() == dev.to_host(b).tobytes() == host.tobytes()
    assert api.hash_usize_to_curve(ctx, DEE, 5, n).tobytes() == host.tobytes()


CASES = ((0, 1, 0, 1), (0, 1, 5, 65), (0, 1, 0, 1 << 11), (0, 16, 0, 17), (2, 16, 0, 5), (2, 1, 0, 33), (1, 1, (1 << 32) - 1, 64), (3, 1, 0, 63), (4, 1, 0, 130))
CHILD = r'''
import hashlib
import numpy as np
from plonky_amd import api
from tests import test_gpu_rescue_h2c as t
h = hashlib.sha256()
for curve, rounds, start, count in t.CASES:
    ctx, _ = t.make_ctx(curve, rounds)
    h.update(api.hash_usize_to_curve(ctx, curve, start, count).tobytes())
    h.update(api.hash_base_field_to_curve(ctx, curve, t.mont_seeds(curve, range(start, start + min(count, 20)))).tobytes())
    ctx.free()
print("DIGEST", h.hexdigest())
'''


@pytest.fixture(scope="module")
def small_set_digest():
    h = hashlib.sha256()
    for curve, rounds, start, count in CASES:
        consts = rr.constants(br.CURVES[curve].base.field_id, 4, rounds)
        exp, _ = ref_points(curve, rounds, consts, range(start, start + count))
        h.update(exp.tobytes())
        h.update(exp[:min(count, 20)].tobytes())
    return h.hexdigest()


def test_the_loop_form_behind_the_knob_gives_the_same_bytes(small_set_digest):
    """knobs are read once: the loop form runs in a process of its own"""
    assert "DIGEST " + small_set_digest in checked_child.run_child(CHILD, PLK_H2C_NAIVE="1")


def test_the_small_set_through_the_checked_build(small_set_digest):
    assert "DIGEST " + small_set_digest in checked_child.run_checked(CHILD)


def test_the_points_commit_like_the_reference_points(torch_dev):
    """the device output goes into msm_precompute and an MSM at 2^8 points, and equals the same MSM over the reference's points"""
    torch, dev = torch_dev
    n = 1 << 8
    ctx, consts = make_ctx(DEE, 16)
    with ctx:
        exp, _ = ref_points(DEE, 16, consts, range(n))  # shares the first seeds with the edge test
        scalars = synth.rand_field(api.CURVE_SCALAR_FIELD[DEE], 0xC0117, n)
        want, wz = api.msm_parallel(DEE, scalars, exp, 8)
        dpre = dev.msm_precompute_dev(DEE, dev.rescue_hash_to_curve_dev(ctx, DEE, n))
        oxy, oz = dev.msm_execute_dev(dpre, dev.to_device(scalars))
        torch.cuda.synchronize()
        assert wz == 0 and int(oz.cpu()[0]) == 0 and np.array_equal(dev.to_host(oxy).reshape(2, -1), want)


def test_refused_arguments_leave_a_pinned_buffer_untouched(torch_dev):
    torch, dev = torch_dev
    pinned = torch.full((8192,), 0x5A5A, dtype=torch.int64).pin_memory()
    L = lib.load()
    P = pinned.data_ptr()
    ctx, _ = make_ctx(DEE, 1)       # TweedledeeBase
    ctx_dum, _ = make_ctx(1, 1)     # TweedledumBase
    H, HD = ctx.handle, ctx_dum.handle
    calls = []
    for text, args_of in (("null context", lambda: (4, None, 0)),
                          ("bad curve id", lambda: (4, H, -1)), ("bad curve id", lambda: (4, H, 5)), ("bad curve id", lambda: (4, H, 99)),
                          ("bad curve id", lambda: (0, H, 5)),  # refused before the count is looked at
                          ("base field", lambda: (4, HD, 0)), ("base field", lambda: (4, H, 1)), ("base field", lambda: (4, H, 2)),
                          ("count", lambda: (1 << 32, H, 0)), ("count", lambda: ((1 << 40) + 3, H, 0))):
        calls += [(text, lambda a=args_of: L.plk_rescue_hash_to_curve(*a(), 0, P)),
                  (text, lambda a=args_of: L.plk_rescue_hash_to_curve_dev(*a(), 0, P, None)),
                  (text, lambda a=args_of: L.plk_rescue_hash_field_to_curve(*a(), P, P)),
                  (text, lambda a=args_of: L.plk_rescue_hash_field_to_curve_dev(*a(), P, P, None))]
    calls += [("null", lambda: L.plk_rescue_hash_to_curve(4, H, 0, 0, None)),
              ("null", lambda: L.plk_rescue_hash_to_curve_dev(4, H, 0, 0, None, None)),
              ("null", lambda: L.plk_rescue_hash_field_to_curve(4, H, 0, None, P)),
              ("null", lambda: L.plk_rescue_hash_field_to_curve(4, H, 0, P, None)),
              ("null", lambda: L.plk_rescue_hash_field_to_curve_dev(4, H, 0, None, P, None)),
              ("null", lambda: L.plk_rescue_hash_field_to_curve_dev(4, H, 0, P, None, None))]
    if torch.cuda.device_count() > 1:  # a context on another device
        with torch.cuda.device(1):
            other, _ = make_ctx(DEE, 1)
        calls += [("lives on device", lambda: L.plk_rescue_hash_to_curve(4, other.handle, 0, 0, P)),
                  ("lives on device", lambda: L.plk_rescue_hash_field_to_curve_dev(4, other.handle, 0, P, P, None))]
    for n, (text, call) in enumerate(calls):
        rc = call()
        err = L.plk_last_error().decode("utf-8", "replace")
        assert rc == lib.PLK_ERR_INVALID_ARG and text in err, (n, text, rc, err)
    torch.cuda.synchronize()
    assert bool((pinned == 0x5A5A).all()), "a refused call wrote"
    # count == 0 is PLK_OK, null pointers and all
    assert L.plk_rescue_hash_to_curve(0, H, 0, 0, None) == 0 and L.plk_rescue_hash_to_curve_dev(0, H, 0, 0, None, None) == 0
    assert L.plk_rescue_hash_field_to_curve(0, H, 0, None, None) == 0 and L.plk_rescue_hash_field_to_curve_dev(0, H, 0, None, None, None) == 0
    with pytest.raises(ValueError):
        api.hash_usize_to_curve(ctx_dum, DEE, 0, 4)
    with pytest.raises(ValueError):
        dev.rescue_hash_to_curve_dev(ctx_dum, DEE, 4)
    with pytest.raises(ValueError):
        dev.rescue_hash_field_to_curve_dev(ctx, 1, torch.zeros((4, 4), dtype=torch.int64, device="cuda"))
    ctx.free()
    ctx_dum.free()
