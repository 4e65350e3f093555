"""GPU parity: what one execution asks of an MSM context - affine or projective result, a bucket share, a batch - must not reach the
next execution on the same context.  The form of the result and the grid of k_msm_heads are options of a call (MsmCall, msm.hip), not
state of the context: this suite runs calls of different kinds back to back on one context and checks every one against big integers.

Generators G_i = G + i D with D = [d] G, so that sum_i s_i G_i = [sum_i s_i (1 + i d) mod r] G: one ec_mul on Python integers
(oracle/bigint_ref.py), bit for bit - affine results are unique.  Tweedledee, n = 6000 at window 16: the two-level reduction, the smallest
shape at which both the projective emit and the wide k_msm_heads grid of a bucket share matter (tests/test_gpu_msm_collisions.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import plonky_amd as pa
from plonky_amd import synth
from oracle import bigint_ref as br

C = br.TWEEDLEDEE
D_MULT = 0xB1A5ED


def _point(P):
    return np.array([C.base.mont_limbs(P[0]), C.base.mont_limbs(P[1])], dtype=np.uint64)


def _setup(dev, n, seeds):
    """device generators G + i D, scalar vectors (Montgomery limbs) and the expected affine points"""
    G = (C.gx, C.gy)
    bases = dev.gen_bases_dev(C.curve_id, n, _point(G), _point(br.ec_mul(C, D_MULT, G)))
    r = C.scalar.p
    vecs, exps = [], []
    for seed in seeds:
        s = synth.rand_field(C.scalar.field_id, seed, n)
        total = sum(C.scalar.from_mont(synth.to_int(row)) * (1 + i * D_MULT) for i, row in enumerate(s)) % r
        vecs.append(s)
        exps.append(_point(br.ec_mul(C, total, G)))
    return bases, vecs, exps


def _to_affine(xyz):
    f = C.base
    x, y, z = (f.from_mont(synth.to_int(xyz[k])) for k in range(3))
    zi = pow(z, -1, f.p)
    return _point((x * zi % f.p, y * zi % f.p))


def test_calls_of_different_kinds_on_one_context():
    pytest.importorskip("torch")
    from plonky_amd import device as dev
    dev.init(0)
    n = 6000
    bases, (s0, s1), (e0, e1) = _setup(dev, n, (0xCA11, 0xCA12))
    pre = dev.msm_precompute_dev(C.curve_id, bases, device_window=16)
    assert pre.window == 16
    d0 = dev.to_device(s0)
    # 1. affine
    oxy, oz = dev.msm_execute_dev(pre, d0)
    first, first_z = dev.to_host(oxy).copy(), oz.cpu().numpy().copy()
    assert int(first_z[0]) == 0 and np.array_equal(first[0], e0)
    # 2. projective: some representative of the same point
    oxyz, oz = dev.msm_execute_dev(pre, d0, projective=True)
    assert int(oz.cpu()[0]) == 0 and np.array_equal(_to_affine(dev.to_host(oxyz)[0]), e0)
    # 3. both halves of the coarse bins in one call: the two shares add up to the whole
    oxy, oz = dev.msm_execute_parts_dev(pre, [(0, d0), (0, d0)], buckets=[(0, 2), (1, 2)])
    shares, sz = dev.to_host(oxy), oz.cpu().numpy()
    assert not np.array_equal(shares[0], e0) and not np.array_equal(shares[1], e0)
    tot, tz = pa.curve_sum_affine(C.curve_id, shares, sz.astype(np.uint8))
    assert tz == 0 and np.array_equal(tot.reshape(e0.shape), e0)
    # 4. a batch of two vectors
    oxy, oz = dev.msm_execute_dev(pre, dev.to_device(np.stack([s0, s1])))
    got, gz = dev.to_host(oxy), oz.cpu().numpy()
    assert list(gz) == [0, 0] and np.array_equal(got[0], e0) and np.array_equal(got[1], e1)
    # 5. the first call again: the same bits
    oxy, oz = dev.msm_execute_dev(pre, d0)
    assert np.array_equal(dev.to_host(oxy), first) and np.array_equal(oz.cpu().numpy(), first_z)
    pre.free()


def test_projective_then_affine_on_a_comb_context():
    """64 generators with an automatic window are a comb (comb.hip), which has no projective form: msm_execute_dev_impl refuses one with
    PLK_ERR_INVALID_ARG, and plk_msm_execute_projective_dev - the one exported entry that asks for projective results - never sends a
    comb context there: it runs the affine execution and returns the point with z = 1.  So through the C ABI the request succeeds; what
    is checked is that it returns the right point, in that form, and that the affine execution after it is right."""
    pytest.importorskip("torch")
    from plonky_amd import device as dev
    dev.init(0)
    n = 64
    bases, (s0,), (e0,) = _setup(dev, n, (0xC0B,))
    pre = dev.msm_precompute_dev(C.curve_id, bases)
    assert pre.window == 4   # the comb's digit width
    d0 = dev.to_device(s0)
    oxyz, oz = dev.msm_execute_dev(pre, d0, projective=True)
    xyz = dev.to_host(oxyz)[0]
    assert int(oz.cpu()[0]) == 0 and np.array_equal(xyz[:2], e0) and C.base.from_mont(synth.to_int(xyz[2])) == 1
    oxy, oz = dev.msm_execute_dev(pre, d0)
    assert int(oz.cpu()[0]) == 0 and np.array_equal(dev.to_host(oxy)[0], e0)
    pre.free()
