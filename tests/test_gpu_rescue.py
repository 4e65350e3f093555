"""Rescue on the device (plonky_amd/csrc/rescue.hip) against tests/rescue_ref.py, word for word: the permutation on all six fields at
the edges of a quad, a wave and a workgroup, the sponge over every absorb / squeeze shape, k-th roots, the Challenger, the refusals,
and the sponge feeding the curve equation.

The Python reference costs about 0.15 ms per round and state, so the states of a batch repeat with a period (67, 5, 37) that shares
no factor with the quad, the wave or the workgroup: every lane position still meets every kind of state, a wrong index still lands on
a different state, and each distinct state is computed once per (field, rounds) and shared."""
import ctypes
from math import gcd

import numpy as np
import pytest

from oracle import bigint_ref as br
from plonky_amd import api, lib, synth
from tests import rescue_ref as rr

pytestmark = pytest.mark.gpu

FIELDS = sorted(br.FIELDS)
COUNTS = (1, 3, 15, 16, 17, 63, 64, 65, 257, 1000)  # a quad is a state, a wave 16 states, a workgroup 64
ROUNDS = (1, 10, 16)
PERIOD = 67
_perm_cache = {}


def mont_rows(field, values):
    return np.stack([synth.mont(field, v) for v in values])


def from_rows(field, rows):
    return [synth.from_mont(field, r) for r in rows]


def pool_states(field):
    """PERIOD states: zero, all p - 1, one-hot in each position (a wrong DPP lane or a transposed matrix shows here), seeded random"""
    p = br.FIELDS[field].p
    fixed = [[0] * 4, [p - 1] * 4] + [[1 if c == e else 0 for c in range(4)] for e in range(4)] + [[(p - 1) if c == e else 0 for c in range(4)] for e in range(4)]
    rnd = from_rows(field, synth.rand_field(field, 0x5E5C + field, 4 * (PERIOD - len(fixed))))
    return fixed + [rnd[4 * i:4 * i + 4] for i in range(PERIOD - len(fixed))]


def make_ctx(field, rounds, seed=1337):
    consts = rr.constants(field, 4, rounds, seed)
    limbs = np.array(rr.constants_limbs(field, consts), dtype=np.uint64).reshape(rounds, 2, 4, -1)
    return api.RescueContext(field, limbs), consts


def ref_perm(field, rounds, consts, state):
    key = (field, rounds, tuple(state))
    if key not in _perm_cache:
        _perm_cache[key] = rr.rescue_permutation(field, state, consts)
    return _perm_cache[key]


def batch(field, rounds, consts, count, shift=0):
    pool = pool_states(field)
    states = [pool[(i + shift) % PERIOD] for i in range(count)]
    inp = np.stack([mont_rows(field, s) for s in pool])[[(i + shift) % PERIOD for i in range(count)]]
    exp_pool = np.stack([mont_rows(field, ref_perm(field, rounds, consts, s)) for s in pool])
    return states, np.ascontiguousarray(inp), np.ascontiguousarray(exp_pool[[(i + shift) % PERIOD for i in range(count)]])


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    return torch, dev


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("field", FIELDS)
def test_permutation_matches_the_reference_word_for_word(field, rounds):
    with make_ctx(field, rounds)[0] as ctx:
        consts = rr.constants(field, 4, rounds)
        for count in COUNTS:
            _, inp, exp = batch(field, rounds, consts, count, shift=count)
            got = api.rescue_permutation(ctx, inp)
            assert got.shape == exp.shape and np.array_equal(got, exp), (field, rounds, count, np.argwhere(got != exp)[:4].tolist())
        one = api.rescue_permutation(ctx, inp[0])  # a single (4, L) state
        assert np.array_equal(one, exp[0])
        assert api.rescue_permutation(ctx, inp[:0]).shape == inp[:0].shape  # count 0: nothing launched


@pytest.mark.parametrize("field", FIELDS)
def test_device_form_in_place_two_streams_and_repeatable(field, torch_dev):
    torch, dev = torch_dev
    rounds = 16
    ctx, consts = make_ctx(field, rounds)
    with ctx:
        _, in_a, exp_a = batch(field, rounds, consts, 65, shift=1)
        _, in_b, exp_b = batch(field, rounds, consts, 257, shift=30)
        ta, tb = dev.to_device(in_a), dev.to_device(in_b)
        torch.cuda.synchronize()
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(sa):
            oa = dev.rescue_permutation_dev(ctx, ta)
        with torch.cuda.stream(sb):
            ob = dev.rescue_permutation_dev(ctx, tb)
        torch.cuda.synchronize()
        assert np.array_equal(dev.to_host(oa), exp_a) and np.array_equal(dev.to_host(ob), exp_b)
        again = dev.rescue_permutation_dev(ctx, ta)
        torch.cuda.synchronize()
        assert torch.equal(again, oa)
        same = dev.rescue_permutation_dev(ctx, tb, out=tb)  # in place
        torch.cuda.synchronize()
        assert same.data_ptr() == tb.data_ptr() and np.array_equal(dev.to_host(tb), exp_b)


def test_more_workgroups_than_the_gpu_holds(torch_dev):
    torch, dev = torch_dev
    field, rounds, n = 0, 16, 1 << 14
    ctx, consts = make_ctx(field, rounds)
    with ctx:
        states = synth.rand_field(field, 0xB16, 4 * n).reshape(n, 4, -1)
        out = dev.rescue_permutation_dev(ctx, dev.to_device(states))
        torch.cuda.synchronize()
        got = dev.to_host(out)
        rows = sorted(set([0, 1, 63, 64, n - 65, n - 1] + [int(v) for v in np.random.default_rng(7).integers(0, n, 140)]))[:128]
        assert len(rows) == 128
        for i in rows:
            exp = rr.rescue_permutation(field, from_rows(field, states[i]), consts)
            assert np.array_equal(got[i], mont_rows(field, exp)), i


SPONGE_IN = (0, 1, 2, 3, 4, 6, 7)
SPONGE_OUT = (1, 2, 3, 4, 7)
SPONGE_PERIOD = 5


def sponge_case(field, consts, n_in, n_out, count, cache):
    p = br.FIELDS[field].p
    rnd = from_rows(field, synth.rand_field(field, 0xAB50 + field, 7 * SPONGE_PERIOD))
    rows = [rnd[7 * r:7 * r + 7] for r in range(SPONGE_PERIOD)]
    rows[1] = [0] * 7
    rows[2] = [p - 1] * 7
    exp_rows = []
    for r in range(SPONGE_PERIOD):
        key = (n_in, n_out, r)
        if key not in cache:
            cache[key] = rr.rescue_sponge(field, rows[r][:n_in], n_out, consts)
        exp_rows.append(cache[key])
    L = synth.LIMBS[field]
    inp = np.zeros((count, n_in, L), dtype=np.uint64)
    exp = np.zeros((count, n_out, L), dtype=np.uint64)
    pool_in = [mont_rows(field, rows[r][:n_in]) if n_in else np.zeros((0, L), dtype=np.uint64) for r in range(SPONGE_PERIOD)]
    pool_exp = [mont_rows(field, e) for e in exp_rows]
    for i in range(count):
        inp[i], exp[i] = pool_in[i % SPONGE_PERIOD], pool_exp[i % SPONGE_PERIOD]
    return inp, exp


@pytest.mark.parametrize("field", FIELDS)
def test_sponge_every_absorb_and_squeeze_shape(field, torch_dev):
    """Two rounds keep the reference quick: the round loop is the permutation's own (covered above at 1, 10 and 16 rounds); what
    this walks is the absorb / squeeze structure - no absorb at all, a short last chunk, a second and a third squeeze block.  The
    widest shape runs once more at the full 16 rounds."""
    torch, dev = torch_dev
    for rounds, shapes in ((2, [(i, o) for i in SPONGE_IN for o in SPONGE_OUT]), (16, [(7, 7)])):
        ctx, consts = make_ctx(field, rounds)
        cache = {}
        with ctx:
            for n_in, n_out in shapes:
                for count in (1, 17, 65):
                    inp, exp = sponge_case(field, consts, n_in, n_out, count, cache)
                    got = api.rescue_sponge(ctx, inp, n_out)
                    assert got.shape == exp.shape and np.array_equal(got, exp), (field, rounds, n_in, n_out, count)
            inp, exp = sponge_case(field, consts, 4, 3, 65, cache)
            out = dev.rescue_sponge_dev(ctx, dev.to_device(inp), 3)
            torch.cuda.synchronize()
            assert np.array_equal(dev.to_host(out), exp)
            h1, h2, h3 = api.rescue_hash_n_to_1(ctx, inp[3]), api.rescue_hash_n_to_2(ctx, inp[3]), api.rescue_hash_n_to_3(ctx, inp[3])
            assert np.array_equal(h3, exp[3]) and np.array_equal(h2, exp[3][:2]) and np.array_equal(h1, exp[3][:1])


ROOT_PERIOD = 37


@pytest.mark.parametrize("field", FIELDS)
def test_kth_roots(field, torch_dev):
    torch, dev = torch_dev
    f = br.FIELDS[field]
    ks = [1, rr.ALPHA[field]] + [k for k in (5, 7, 11, 13) if gcd(k, f.p - 1) == 1]
    assert set(ks) == ({1, 11} if field == 2 else {1, 5, 11} if field == 3 else {1, 5, 7, 11, 13})
    pool = [0, 1, f.p - 1] + from_rows(field, synth.rand_field(field, 0x4007 + field, ROOT_PERIOD - 3))
    pool_m = mont_rows(field, pool)
    for k in ks:
        exp_pool = [rr.kth_root(f.p, x, k) for x in pool]
        assert all(pow(y, k, f.p) == x for x, y in zip(pool, exp_pool))
        exp_m = mont_rows(field, exp_pool)
        for count in (1, 64, 65, 1000):
            idx = [(i + count) % ROOT_PERIOD for i in range(count)]
            got = api.kth_root(field, pool_m[idx], k)
            assert np.array_equal(got, exp_m[idx]), (field, k, count)
        ys = from_rows(field, got[:ROOT_PERIOD])
        assert all(pow(y, k, f.p) == pool[j] for y, j in zip(ys, idx[:ROOT_PERIOD]))  # out^k == in
        t = dev.to_device(np.ascontiguousarray(pool_m[idx]))
        dev.kth_root_dev(field, t, k, out=t)
        torch.cuda.synchronize()
        assert np.array_equal(dev.to_host(t), exp_m[idx])


@pytest.mark.parametrize("field", (0, 3))
def test_challenger_script(field):
    f = br.FIELDS[field]
    rounds = api.rescue_rounds(4, 128)
    assert rounds == 16 and api.rescue_rounds(4, 64) == 10
    ctx, consts = make_ctx(field, rounds)
    with ctx:
        vals = from_rows(field, synth.rand_field(field, 0xC4A1 + field, 24))
        m = lambda v: synth.mont(field, v)  # noqa: E731
        dev_c, ref_c = api.Challenger(ctx), rr.Challenger(field, consts)
        # 1. observe 18 elements, two challenges
        dev_c.observe_elements([m(v) for v in vals[:18]])
        ref_c.observe_elements(vals[:18])
        got, exp = dev_c.get_2_challenges(), ref_c.get_2_challenges()
        assert from_rows(field, got) == list(exp) and exp[0] == exp[1]
        # 2. observe a point, one challenge
        dev_c.observe_affine_point(np.stack([m(vals[18]), m(vals[19])]))
        ref_c.observe_affine_point((vals[18], vals[19]))
        e2 = ref_c.get_challenge()
        assert synth.from_mont(field, dev_c.get_challenge()) == e2 and e2 != exp[0]
        # 3. three challenges in a row, no observation: the reference's behaviour, kept
        got3, exp3 = dev_c.get_3_challenges(), ref_c.get_3_challenges()
        assert from_rows(field, got3) == list(exp3) == [e2] * 3
        assert from_rows(field, dev_c.get_n_challenges(2)) == ref_c.get_n_challenges(2)
        # 4. clone, diverge the clone, the original is untouched
        dev_d, ref_d = dev_c.clone(), ref_c.clone()
        dev_d.observe_element(m(vals[20]))
        ref_d.observe_element(vals[20])
        ed = ref_d.get_challenge()
        assert synth.from_mont(field, dev_d.get_challenge()) == ed and ed != e2
        assert synth.from_mont(field, dev_c.get_challenge()) == ref_c.get_challenge() == e2
        assert all(0 <= v < f.p for v in (ed, e2))


def test_mds_entry(torch_dev):
    for field in FIELDS:
        got = api.rescue_mds(field)
        exp = np.stack([mont_rows(field, row) for row in rr.mds_matrix(br.FIELDS[field].p, 4)])
        assert np.array_equal(got, exp), field


@pytest.fixture(scope="module")
def pinned(torch_dev):
    """64 KiB of pinned memory that host and device can both address, with a pattern no refused call may disturb"""
    torch, _ = torch_dev
    return torch.full((8192,), 0x5A5A, dtype=torch.int64).pin_memory()


def test_refused_arguments(pinned, torch_dev):
    torch, _ = torch_dev
    L = lib.load()
    P = pinned.data_ptr()
    ctx, _ = make_ctx(0, 1)
    ctx2, _ = make_ctx(2, 1)
    H, H2 = ctx.handle, ctx2.handle
    out_ctx = ctypes.c_void_p()
    calls = []
    for field in (-1, 6, 1000):  # an unknown field id
        calls += [("bad field id", lambda f=field: L.plk_rescue_create(4, f, 1, P, ctypes.byref(out_ctx))),
                  ("bad field id", lambda f=field: L.plk_rescue_mds(4, f, P)),
                  ("bad field id", lambda f=field: L.plk_field_kth_root(4, f, 5, P, P)),
                  ("bad field id", lambda f=field: L.plk_field_kth_root_dev(4, f, 5, P, P, None))]
    for width in (0, 3, 5, 8):  # width != 4
        calls += [("width", lambda w=width: L.plk_rescue_create(w, 0, 1, P, ctypes.byref(out_ctx))),
                  ("width", lambda w=width: L.plk_rescue_mds(w, 0, P))]
    calls += [("rounds", lambda: L.plk_rescue_create(4, 0, 0, P, ctypes.byref(out_ctx))),
              ("null", lambda: L.plk_rescue_create(4, 0, 1, None, ctypes.byref(out_ctx))),
              ("null", lambda: L.plk_rescue_create(4, 0, 1, P, None)),
              ("null", lambda: L.plk_rescue_mds(4, 0, None)),
              # a null context
              ("null context", lambda: L.plk_rescue_permutation(4, None, P, P)),
              ("null context", lambda: L.plk_rescue_permutation_dev(4, None, P, P, None)),
              ("null context", lambda: L.plk_rescue_sponge(4, None, 2, P, 2, P)),
              ("null context", lambda: L.plk_rescue_sponge_dev(4, None, 2, P, 2, P, None)),
              # a null pointer with count > 0
              ("null", lambda: L.plk_rescue_permutation(4, H, None, P)),
              ("null", lambda: L.plk_rescue_permutation(4, H, P, None)),
              ("null", lambda: L.plk_rescue_permutation_dev(4, H, None, P, None)),
              ("null", lambda: L.plk_rescue_permutation_dev(4, H, P, None, None)),
              ("null", lambda: L.plk_rescue_sponge(4, H, 2, None, 2, P)),
              ("null", lambda: L.plk_rescue_sponge(4, H, 2, P, 2, None)),
              ("null", lambda: L.plk_rescue_sponge_dev(4, H, 2, None, 2, P, None)),
              ("null", lambda: L.plk_rescue_sponge_dev(4, H, 0, None, 2, None, None)),
              ("null", lambda: L.plk_field_kth_root(4, 0, 5, None, P)),
              ("null", lambda: L.plk_field_kth_root(4, 0, 5, P, None)),
              ("null", lambda: L.plk_field_kth_root_dev(4, 0, 5, None, P, None)),
              ("null", lambda: L.plk_field_kth_root_dev(4, 0, 5, P, None, None)),
              # n_outputs == 0
              ("n_outputs", lambda: L.plk_rescue_sponge(4, H, 2, P, 0, P)),
              ("n_outputs", lambda: L.plk_rescue_sponge_dev(4, H2, 2, P, 0, P, None)),
              # k = 0
              ("k = 0", lambda: L.plk_field_kth_root(4, 0, 0, P, P)),
              ("k = 0", lambda: L.plk_field_kth_root_dev(4, 0, 0, P, P, None))]
    for field in FIELDS:  # gcd(k, p - 1) != 1: 3 everywhere, 5 and 7 on Bls12377Scalar, 7 and 13 on Bls12377Base
        for k in [3] + ([5, 7, 13] if field == 2 else [7, 13] if field == 3 else []):
            assert gcd(k, br.FIELDS[field].p - 1) != 1
            calls += [("does not permute", lambda f=field, kk=k: L.plk_field_kth_root(4, f, kk, P, P)),
                      ("does not permute", lambda f=field, kk=k: L.plk_field_kth_root_dev(4, f, kk, P, P, None))]
    for n, (text, call) in enumerate(calls):
        rc = call()
        err = L.plk_last_error().decode("utf-8", "replace")
        assert rc == lib.PLK_ERR_INVALID_ARG and text in err, (n, text, rc, err)
        assert not out_ctx.value, n
    torch.cuda.synchronize()
    assert bool((pinned == 0x5A5A).all()), "a refused call wrote"
    # count == 0 is PLK_OK, null pointers and all
    assert L.plk_rescue_permutation(0, H, None, None) == 0 and L.plk_rescue_sponge_dev(0, H, 2, None, 2, None, None) == 0
    assert L.plk_field_kth_root(0, 0, 5, None, None) == 0
    with pytest.raises(ValueError):
        api.kth_root(0, np.zeros((1, 4), dtype=np.uint64), 3)
    ctx.free()
    ctx2.free()


def test_sponge_feeds_the_curve_equation(torch_dev):
    """The shape of hash_base_field_to_curve (hash_to_curve.rs:78-104): hash (seed, i) to two elements and try x in the curve
    equation.  About half of all x have a square x^3 + B; a share outside 0.4 .. 0.6 over 2^10 seeds (eight standard deviations)
    would mean the sponge's outputs are not spread over the field.  Not an implementation of that function."""
    torch, dev = torch_dev
    curve = br.CURVES[0]
    field, p, n = curve.base.field_id, curve.base.p, 1 << 10
    ctx, consts = make_ctx(field, 16)
    with ctx:
        pairs = [(seed, seed % 3) for seed in range(n)]
        inp = np.stack([mont_rows(field, pr) for pr in pairs])
        out = dev.rescue_sponge_dev(ctx, dev.to_device(inp), 2)
        torch.cuda.synchronize()
        got = dev.to_host(out)
        for i in (0, 1, 513, n - 1):
            assert from_rows(field, got[i]) == rr.rescue_sponge(field, list(pairs[i]), 2, consts), i
        xs = [synth.from_mont(field, row[0]) for row in got]
        squares = sum(1 for x in xs if pow((x * x * x + curve.b) % p, (p - 1) // 2, p) in (0, 1))
        assert len(set(xs)) == n
        assert 0.4 <= squares / n <= 0.6, squares
