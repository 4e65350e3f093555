"""GPU parity: k_ntt_pass on the inputs a witness is made of, and on every zero-padding ratio.

No reduction happens inside a tile of the pass kernel (ntt.hip): a value grows by up to 2p per stage, carries move twice per radix-4
step, the first step takes x2 + x3 off 4p, and the last pass ends with fz_reduce_small and ONE conditional subtraction.  Seeded random
elements sit in the middle of every one of those windows.  The case table (tests/ntt_structured_cases.py, pinned on the host by
tests/test_ntt_structured_cases.py) holds the other end: exact zeros, butterflies of equal operands, -1 at every stage, limbs that are
all ones or all zeros, Montgomery words next to every limb boundary - through every tile height 1 .. 10 as a first, a middle and a last
pass, forward and inverse, one transform at a time and in a batch.

The zero-padded transform (fft_with_precomputation, fft.rs:60-80) skips the stages that would pair a value with a zero: the first pass
starts at stage `skip`, found from the input length (run_plan_t).  Every skip from 0 (no padding) to log_a (no stage at all) is run here
on both sides of its threshold, an odd skip (which moves the radix-2 tail) as well as an even one, the empty input, and a batch whose
rows are further apart than they are long.

Every comparison is bit exact against the oracle (one representation per element, so canonical outputs are implied); cases with a
closed form are compared with it as well."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import plonky_amd as pa
from plonky_amd import api, lib
from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from tests import ntt_structured_cases as nsc
from tests.test_gpu_ntt_plans import _restore_plan_rule, _with_plan  # noqa: F401  (the fixture is autouse here too)
from tests.test_oracle_kats import mont_arr

ALL_FIELDS = list(br.FIELDS.values())
PLAN_FIELDS = [br.TWEEDLEDEE_BASE, br.BLS12_377_SCALAR, br.PALLAS_BASE, br.BLS12_377_BASE]
PAD_FIELDS = [br.TWEEDLEDEE_BASE, br.BLS12_377_BASE]
DEFAULT_LOG_NS = [1, 2, 3, 5, 8, 10, 12, 14]
# the smallest sizes that reach every tile height 1 .. 10 as a first, a middle and a last pass
PLANS = {
    10: ["10"],
    11: ["10,1", "1,10", "6,5"],
    13: ["10,3", "3,10", "7,6", "9,4", "2,2,2,7"],
    16: ["10,6", "6,10", "8,8", "7,9", "4,4,4,4"],
}

_words = {}  # field id -> {canonical value: the bytes of its Montgomery words}


def _closed_array(f, vals):
    """mont_arr(f, vals); the conversion of a value is done once per field (the closed forms repeat a few values, or powers of w)"""
    uniq = set(vals)
    if len(uniq) <= 2:  # a constant, or one value among zeros
        major = max(uniq, key=vals.count)
        rows = dict(zip(uniq, mont_arr(f, list(uniq))))
        out = np.repeat(rows[major][None, :], len(vals), axis=0)
        for v in uniq - {major}:
            out[[i for i, w in enumerate(vals) if w == v]] = rows[v]
        return out
    memo = _words.setdefault(f.field_id, {})
    new = [v for v in uniq if v not in memo]
    for v, row in zip(new, mont_arr(f, new) if new else ()):
        memo[v] = row.tobytes()
    return np.frombuffer(b"".join([memo[v] for v in vals]), dtype=np.uint64).reshape(len(vals), f.n_limbs)


@functools.lru_cache(maxsize=1)
def _expected(field_id, log_n):
    """case name -> (oracle forward, oracle inverse, closed forward or None, closed inverse or None); computed once, never written to.
    The oracle's transforms are independent calls into its library: a few host threads share them."""
    f = br.FIELDS[field_id]
    opre = ol.FftPrecomputation(field_id, 1 << log_n)
    cs = nsc.cases(field_id, log_n)
    with ThreadPoolExecutor(max_workers=8) as pool:
        fwd = pool.map(lambda c: opre.fft_with_precomputation_power_of_2(c.x), cs)
        inv = pool.map(lambda c: opre.ifft_with_precomputation_power_of_2(c.x), cs)
        closed = [(None if c.fwd is None else _closed_array(f, c.fwd()), None if c.inv is None else _closed_array(f, c.inv())) for c in cs]
        out = {c.name: (a, b) + cl for c, a, b, cl in zip(cs, fwd, inv, closed)}
    _words.pop(field_id, None)
    return out


def _launches_of(call):
    """(result of call(), launches of the pass kernel it made)"""
    L = lib.load()
    ms, launches = ctypes.c_double(), ctypes.c_uint()
    lib.check(L.plk_ntt_set_profiling(1))
    try:
        got = call()
        lib.check(L.plk_ntt_get_timings(ctypes.byref(ms), ctypes.byref(launches)))
    finally:
        lib.check(L.plk_ntt_set_profiling(0))
    return got, launches.value


def _check_every_case(f, log_n, tag):
    pre = pa.fft_precompute(f.field_id, 1 << log_n)
    exp = _expected(f.field_id, log_n)
    for c in nsc.cases(f.field_id, log_n):
        exp_fwd, exp_inv, closed_fwd, closed_inv = exp[c.name]
        fwd = pa.fft_with_precomputation_power_of_2(c.x, pre)
        inv = pa.ifft_with_precomputation_power_of_2(c.x, pre)
        assert np.array_equal(fwd, exp_fwd), (tag, c.name, "forward")
        assert np.array_equal(inv, exp_inv), (tag, c.name, "inverse")
        if closed_fwd is not None:
            assert np.array_equal(fwd, closed_fwd), (tag, c.name, "forward, closed form")
            assert np.array_equal(inv, closed_inv), (tag, c.name, "inverse, closed form")
        assert np.array_equal(pa.ifft_with_precomputation_power_of_2(fwd, pre), c.x), (tag, c.name, "round trip")


# ---- a. structured values through every tile height ----
@pytest.mark.parametrize("f", ALL_FIELDS, ids=lambda f: f.name)
@pytest.mark.parametrize("log_n", DEFAULT_LOG_NS)
def test_structured_ntt_default_plan(f, log_n):
    _with_plan(None)
    _check_every_case(f, log_n, "default")


@pytest.mark.parametrize("f", PLAN_FIELDS, ids=lambda f: f.name)
@pytest.mark.parametrize("log_n", sorted(PLANS))
def test_structured_ntt_chosen_plans(f, log_n):
    x = nsc.case(f.field_id, log_n, "delta(0,p-1)").x
    for plan in PLANS[log_n]:
        _with_plan(plan)
        pre = pa.fft_precompute(f.field_id, 1 << log_n)
        # the plan really is the one asked for: one launch of the pass kernel per pass
        _, launches = _launches_of(lambda: pa.fft_with_precomputation_power_of_2(x, pre))
        assert launches == len(plan.split(",")), (plan, launches)
        _check_every_case(f, log_n, plan)


BATCH_LOG_N = 13
BATCH_ROWS = ["zero", "delta(0,p-1)", "constant(p-1)", "raw_cycle"]


@pytest.mark.parametrize("f", [br.TWEEDLEDEE_BASE, br.BLS12_377_BASE], ids=lambda f: f.name)
def test_structured_ntt_batch_rows_match_single_transforms(f):
    from plonky_amd import device as dev
    dev.init(0)
    log_n = BATCH_LOG_N
    rows = [nsc.case(f.field_id, log_n, name).x for name in BATCH_ROWS] + [nsc.random_vector(f, log_n, salt=2)]
    stack = np.ascontiguousarray(np.stack(rows))
    pre = pa.fft_precompute(f.field_id, 1 << log_n)
    opre = ol.FftPrecomputation(f.field_id, 1 << log_n)
    d_stack = dev.to_device(stack)
    for inverse in (False, True):
        one = pa.ifft_with_precomputation_power_of_2 if inverse else pa.fft_with_precomputation_power_of_2
        orc = opre.ifft_with_precomputation_power_of_2 if inverse else opre.fft_with_precomputation_power_of_2
        host = api.fft_batch(f.field_id, stack, inverse=inverse)
        on_dev = dev.to_host(dev.ntt_dev(f.field_id, d_stack, inverse=inverse))
        for k, x in enumerate(rows):
            single = one(x, pre)
            assert np.array_equal(single, orc(x, threads=4)), (k, inverse)
            assert np.array_equal(host[k], single), ("fft_batch", k, inverse)
            assert np.array_equal(on_dev[k], single), ("ntt_dev", k, inverse)
    assert np.array_equal(dev.to_host(d_stack), stack)  # the inputs are where they were


# ---- b. every padding ratio ----
PAD_PLANS = [(13, None), (13, "10,3"), (13, "3,10"), (13, "7,6"), (13, "6,7"), (10, "10")]
MAX_TILE_LOG = 10  # the product's own rule (plan None) never takes a taller first pass


def _pad_sources(f, log_n):
    return {"random": nsc.random_vector(f, log_n, salt=1), "raw_cycle": nsc.pattern_cycle(f, 1 << log_n)}


@functools.lru_cache(maxsize=2)
def _padded_expected(field_id, log_n):
    """(source, in_len) -> the oracle's transform of the first in_len entries followed by zeros, for every length any plan asks for"""
    f = br.FIELDS[field_id]
    n = 1 << log_n
    opre = ol.FftPrecomputation(field_id, n)
    out = {}
    for kind, src in _pad_sources(f, log_n).items():
        for in_len in nsc.padded_lengths(log_n, MAX_TILE_LOG):
            out[kind, in_len] = opre.fft_with_precomputation_power_of_2(nsc.padded(src[:in_len], n), threads=4)
            if in_len > n // 2:  # the reference's own call, where it pads to the same size
                assert np.array_equal(opre.fft_with_precomputation(np.ascontiguousarray(src[:in_len]), threads=4), out[kind, in_len])
    return out


@pytest.mark.parametrize("f", PAD_FIELDS, ids=lambda f: f.name)
@pytest.mark.parametrize("log_n,plan", PAD_PLANS, ids=["2p%d-%s" % (l, p or "default") for l, p in PAD_PLANS])
def test_padded_lengths_match_oracle(f, log_n, plan):
    from plonky_amd import device as dev
    dev.init(0)
    n, L = 1 << log_n, lib.load()
    first = MAX_TILE_LOG if plan is None else int(plan.split(",")[0])
    lens = nsc.padded_lengths(log_n, first)
    assert {nsc.skipped_stages(log_n, first, v) for v in lens if v} >= set(range(first + 1))
    exp = _padded_expected(f.field_id, log_n)
    _with_plan(plan)
    for kind, src in _pad_sources(f, log_n).items():
        d_src = dev.to_device(src)
        for in_len in lens:
            want = exp[kind, in_len]
            tag = (plan, kind, in_len, "skip %d" % nsc.skipped_stages(log_n, first, in_len))
            assert in_len > 0 or not want.any()
            short = np.ascontiguousarray(src[:in_len])
            # the output buffers start out as non-zero elements: an empty input must overwrite them with zeros, not transform them
            got = np.full((n, f.n_limbs), 0x0123456789ABCDEF, dtype=np.uint64)
            lib.check(L.plk_ntt_padded(f.field_id, log_n, short.ctypes.data_as(ctypes.c_void_p), in_len, got.ctypes.data_as(ctypes.c_void_p)))
            assert np.array_equal(got, want), ("plk_ntt_padded",) + tag
            d_out = dev.to_device(np.full((n, f.n_limbs), 0x0123456789ABCDEF, dtype=np.uint64))
            ret = dev.ntt_padded_dev(f.field_id, d_src[:in_len], log_n, out=d_out)
            assert ret.data_ptr() == d_out.data_ptr()
            assert np.array_equal(dev.to_host(d_out), want), ("ntt_padded_dev",) + tag
        assert np.array_equal(dev.to_host(d_src), src)


# ---- c. batch shapes of the padded entry points ----
@pytest.mark.parametrize("f", PAD_FIELDS, ids=lambda f: f.name)
def test_padded_dev_rows_further_apart_than_long(f):
    """plk_ntt_padded_dev with in_stride != in_len: rows are views into one (3, L + 5) tensor whose trailing columns are not zero"""
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    log_n, batch, gap = 12, 3, 5
    n, lb = 1 << log_n, lib.load()
    opre = ol.FftPrecomputation(f.field_id, n)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for length in (1, n // 8, n // 2 + 1):
        stride = length + gap
        host = nsc.random_vector(f, 14, salt=3 + length % 7)[: batch * stride].reshape(batch, stride, f.n_limbs).copy()
        host[1, : min(length, 4)] = nsc.pattern_cycle(f, 4)[: min(length, 4)]
        assert host[:, length:].any(axis=2).all()
        d_in = dev.to_device(host)
        d_out = torch.empty((batch, n, f.n_limbs), dtype=torch.int64, device="cuda")
        lib.check(lb.plk_ntt_padded_dev(f.field_id, log_n, batch, ctypes.c_void_p(d_in.data_ptr()), length, stride,
                                        ctypes.c_void_p(d_out.data_ptr()), stream))
        got = dev.to_host(d_out)
        for b in range(batch):
            want = opre.fft_with_precomputation_power_of_2(nsc.padded(host[b, :length], n), threads=4)
            assert np.array_equal(got[b], want), (length, b)
        assert np.array_equal(dev.to_host(d_in), host)
        # rows that would overlap are refused; one row has no stride to speak of
        args = (ctypes.c_void_p(d_in.data_ptr()), length, length - 1, ctypes.c_void_p(d_out.data_ptr()), stream)
        assert lb.plk_ntt_padded_dev(f.field_id, log_n, batch, *args) == lib.PLK_ERR_INVALID_ARG
        assert lb.plk_ntt_padded_dev(f.field_id, log_n, 2, *args) == lib.PLK_ERR_INVALID_ARG
        lib.check(lb.plk_ntt_padded_dev(f.field_id, log_n, 1, *args))
        assert np.array_equal(dev.to_host(d_out)[0], got[0]), length


@pytest.mark.parametrize("f", PAD_FIELDS, ids=lambda f: f.name)
def test_padded_batch_of_mixed_lengths(f):
    """plk_ntt_padded_batch: the rows of one call share the longest row's length on the device; the shorter ones are filled with zeros"""
    log_n = 12
    n = 1 << log_n
    lens = (0, 1, n // 8, n // 2 + 1, n)
    opre = ol.FftPrecomputation(f.field_id, n)
    srcs = [nsc.random_vector(f, log_n, salt=10 + b) for b in range(len(lens))]
    srcs[2] = nsc.pattern_cycle(f, n)
    ins_h = [np.ascontiguousarray(s[:v]) for s, v in zip(srcs, lens)]
    out = np.full((len(lens), n, f.n_limbs), 0x0123456789ABCDEF, dtype=np.uint64)
    ins = (ctypes.c_void_p * len(lens))(*[a.ctypes.data for a in ins_h])
    n_in = (ctypes.c_size_t * len(lens))(*lens)
    outs = (ctypes.c_void_p * len(lens))(*[out[b].ctypes.data for b in range(len(lens))])
    lib.check(lib.load().plk_ntt_padded_batch(f.field_id, log_n, len(lens), ins, n_in, outs))
    assert not out[0].any()
    for b, a in enumerate(ins_h):
        assert np.array_equal(out[b], opre.fft_with_precomputation_power_of_2(nsc.padded(a, n), threads=4)), lens[b]
