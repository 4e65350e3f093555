"""GPU: the host-pointer entry points as an untouched caller uses them (plonk_util.rs:169-190): buffers that are slices of larger
allocations - oddly placed, in place, adjacent, overlapping, shared between threads, or registered with the runtime by the caller.

Every buffer lies in an arena whose words are first set to a poison pattern that is no canonical field element; after a call the
output equals the oracle bit for bit, a separate input is unchanged, and every other word of every arena is still poison.  The route
a call took through host_lane.h / pin_registry.h is read from the library's own counters (plk_internal_host_stats) and asserted, so
that a case keeps reaching the path it was written for:
  * copies: staged through the lane's pinned buffer below 64 KiB, direct from 64 KiB on, bounced in chunks when the runtime rejects
    a direct copy;
  * registry: plk_ntt and plk_msm_execute (ONE buffer per direction) never register; the batched calls from 1 MiB per buffer on, the
    padded transform and the polynomial division do - fresh / shared / union as the buffers lie.
"""
import ctypes
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from plonky_amd import lib, synth

POISON = 0xA5A5A5A5A5A5A5A5  # top limb above every modulus here: not a canonical element
PAGE_WORDS = 512
F = 0        # TweedledeeBase, 4 limbs
F_BLS = 3    # Bls12377Base, 6 limbs
STAT_NAMES = ["none", "fresh", "register-failed", "shared", "union", "union-failed", "gave-up", "released-last", "released-kept",
              "release-not-held", "release-unknown", "waits", "rechecks", "staged", "direct", "bounced"]


def arena(words, dtype=np.uint64):
    """`words` poisoned items starting on a page boundary"""
    item = np.dtype(dtype).itemsize
    raw = np.empty(words + 4096 // item, dtype=dtype)
    skip = (-raw.ctypes.data % 4096) // item
    a = raw[skip:skip + words]
    a[:] = POISON if dtype == np.uint64 else 0xA5
    assert a.ctypes.data % 4096 == 0
    return a


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def only_poison(a, *holes):
    """every item of arena `a` outside the [lo, hi) holes is poison"""
    mask = np.ones(a.shape[0], dtype=bool)
    for lo, hi in holes:
        mask[lo:hi] = False
    want = POISON if a.dtype == np.uint64 else 0xA5
    return bool((a[mask] == want).all())


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401
    from plonky_amd import device as dev
    dev.init(0)
    L = lib.load()
    L.plk_internal_host_stats.restype = ctypes.c_int
    L.plk_internal_host_stats.argtypes = [ctypes.c_void_p, ctypes.c_uint]
    assert L.plk_internal_host_stats(None, 0) == len(STAT_NAMES)
    return L


def stats(L):
    v = (ctypes.c_ulonglong * len(STAT_NAMES))()
    L.plk_internal_host_stats(v, len(STAT_NAMES))
    return dict(zip(STAT_NAMES, v))


def delta(L, before):
    """the counters that moved since `before`, releases left out (they mirror the acquires)"""
    now = stats(L)
    return {k: now[k] - before[k] for k in STAT_NAMES if now[k] != before[k] and not k.startswith("release")}


_refs = {}


def vec(field, log_n, seed, count=None):
    """(input, oracle transform of the input zero-padded to 2^log_n), computed once per module"""
    key = (field, log_n, seed, count)
    if key not in _refs:
        n = 1 << log_n
        x = synth.rand_field(field, seed, n if count is None else count)
        full = x
        if x.shape[0] < n:
            full = np.zeros((n, x.shape[1]), dtype=np.uint64)
            full[:x.shape[0]] = x
        y = ol.FftPrecomputation(field, n).fft_with_precomputation_power_of_2(full)
        x.setflags(write=False)
        y.setflags(write=False)
        _refs[key] = (x, y)
    return _refs[key]


@pytest.fixture(scope="module")
def msm(L):
    """one Tweedledee context over 2^15 generators, a scalar vector, the oracle's result"""
    c = br.TWEEDLEDEE
    n = 1 << 15
    G = (c.gx, c.gy)
    pt = lambda P: np.array([c.base.mont_limbs(P[0]), c.base.mont_limbs(P[1])], dtype=np.uint64)  # noqa: E731
    bases = ol.gen_bases(0, n, pt(G), pt(br.ec_mul(c, 0xB0FF01, G)))
    s = synth.rand_field(1, 0xB0FF02, n)
    exp, ez = ol.MsmPrecomputation(0, bases, 8, threads=8).execute(s, parallel=True, threads=8)
    ctx = ctypes.c_void_p()
    lib.check(L.plk_msm_precompute(0, n, ptr(bases), None, 0, ctypes.byref(ctx)))
    yield ctx, s, exp, ez
    L.plk_msm_free(ctx)


# ---- guard bytes and odd placement ----
@pytest.mark.parametrize("in_place", [False, True], ids=["separate", "in_place"])
@pytest.mark.parametrize("field,log_n,route", [(F, 10, "staged"), (F, 11, "direct"), (F, 15, "direct"), (F_BLS, 10, "staged")],
                         ids=["2^10", "2^11", "2^15", "bls12_377_base_2^10"])
def test_ntt_guard_bytes(L, field, log_n, route, in_place):
    """plk_ntt, input and output 8 bytes past a page boundary.  One buffer per direction: 32 KiB (48 KiB on the 48-byte field) is
    staged, 64 KiB and 1 MiB are copied directly, and nothing is registered - a single transform's copies block the caller anyway."""
    x, y = vec(field, log_n, 0x6A0000 + log_n)
    w = x.size
    pages = (w + 1 + PAGE_WORDS - 1) // PAGE_WORDS + 1
    a = arena((2 * pages + 1) * PAGE_WORDS)
    i0 = PAGE_WORDS + 1
    o0 = i0 if in_place else (1 + pages) * PAGE_WORDS + 1
    a[i0:i0 + w] = x.reshape(-1)
    before = stats(L)
    lib.check(L.plk_ntt(field, log_n, 0, ptr(a[i0:]), ptr(a[o0:])))
    assert delta(L, before) == {route: 2}
    assert np.array_equal(a[o0:o0 + w].reshape(y.shape), y)
    if not in_place:
        assert np.array_equal(a[i0:i0 + w].reshape(x.shape), x), "the input was changed"
    assert only_poison(a, (i0, i0 + w), (o0, o0 + w))


@pytest.mark.parametrize("in_place", [False, True], ids=["separate", "in_place"])
def test_ntt_batch_guard_bytes_registered(L, in_place):
    """plk_ntt_batch of two 1 MiB transforms: every buffer is registered for the call (fresh: they do not touch), copied directly."""
    log_n = 15
    refs = [vec(F, log_n, 0x6B0000 + b) for b in range(2)]
    w = refs[0][0].size
    step = w + 2 * PAGE_WORDS
    a = arena(4 * step + PAGE_WORDS)
    ins = [PAGE_WORDS + 1 + b * step for b in range(2)]
    outs = ins if in_place else [PAGE_WORDS + 1 + (2 + b) * step for b in range(2)]
    for b in range(2):
        a[ins[b]:ins[b] + w] = refs[b][0].reshape(-1)
    pi = (ctypes.c_void_p * 2)(*[a[i:].ctypes.data for i in ins])
    po = (ctypes.c_void_p * 2)(*[a[o:].ctypes.data for o in outs])
    before = stats(L)
    lib.check(L.plk_ntt_batch(F, log_n, 0, 2, pi, po))
    assert delta(L, before) == {"fresh": 2 if in_place else 4, "direct": 4}
    for b in range(2):
        assert np.array_equal(a[outs[b]:outs[b] + w].reshape(-1, 4), refs[b][1])
        if not in_place:
            assert np.array_equal(a[ins[b]:ins[b] + w].reshape(-1, 4), refs[b][0])
    assert only_poison(a, *[(i, i + w) for i in ins + outs])
    assert stats(L)["released-last"] - before["released-last"] == (2 if in_place else 4)


@pytest.mark.parametrize("in_place", [False, True], ids=["separate", "in_place"])
@pytest.mark.parametrize("log_n,n_in", [(15, (1 << 15) - 5), (16, (1 << 15) + 3)], ids=["2^15", "2^16"])
def test_ntt_padded_guard_bytes(L, log_n, n_in, in_place):
    """plk_ntt_padded with n_in < n.  Separate: the output is registered, the input only from 1 MiB on.  In place: ONE registration
    of the larger range, and the output's request lies inside it (shared)."""
    x, y = vec(F, log_n, 0x6C0000 + log_n, n_in)
    n = 1 << log_n
    pages = 4 * n // PAGE_WORDS + 2
    a = arena((2 * pages + 1) * PAGE_WORDS)
    i0 = PAGE_WORDS + 1
    o0 = i0 if in_place else (1 + pages) * PAGE_WORDS + 1
    a[i0:i0 + 4 * n_in] = x.reshape(-1)
    before = stats(L)
    lib.check(L.plk_ntt_padded(F, log_n, ptr(a[i0:]), n_in, ptr(a[o0:])))
    if in_place:
        assert delta(L, before) == {"fresh": 1, "shared": 1, "direct": 2}
    else:
        assert delta(L, before) == {"fresh": 2 if n_in * 32 >= 1 << 20 else 1, "direct": 2}
    assert np.array_equal(a[o0:o0 + 4 * n].reshape(n, 4), y)
    if in_place:
        assert only_poison(a, (o0, o0 + 4 * n))
    else:
        assert np.array_equal(a[i0:i0 + 4 * n_in].reshape(n_in, 4), x), "the input was changed"
        assert only_poison(a, (i0, i0 + 4 * n_in), (o0, o0 + 4 * n))


def test_msm_execute_guard_bytes(L, msm):
    """plk_msm_execute, 2^15 scalars: the 1 MiB scalar vector directly (one vector: not registered), the 64-byte point and the
    one-byte flag staged, each into the middle of a poisoned arena."""
    ctx, s, exp, ez = msm
    sa = arena(s.size + 3 * PAGE_WORDS)
    s0 = PAGE_WORDS + 1
    sa[s0:s0 + s.size] = s.reshape(-1)
    xy, zero = arena(2 * PAGE_WORDS), arena(8192, np.uint8)
    x0, z0 = PAGE_WORDS + 1, 4096 + 3
    before = stats(L)
    lib.check(L.plk_msm_execute(ctx, ptr(sa[s0:]), 1 << 15, ptr(xy[x0:]), ptr(zero[z0:])))
    assert delta(L, before) == {"direct": 1, "staged": 2}
    assert np.array_equal(xy[x0:x0 + 8].reshape(2, 4), exp) and int(zero[z0]) == ez
    assert np.array_equal(sa[s0:s0 + s.size].reshape(s.shape), s), "the scalars were changed"
    assert only_poison(sa, (s0, s0 + s.size)) and only_poison(xy, (x0, x0 + 8)) and only_poison(zero, (z0, z0 + 1))


def test_poly_division_guard_bytes(L):
    """plk_poly_division: a and q (1 MiB each) are registered and copied directly, the 64-byte remainder is staged."""
    from tests.test_gpu_poly_division import ints_to_words, ref_divide_stored, words_to_ints
    f = br.TWEEDLEDEE_BASE
    k, q_len = 2, 1 << 15
    la = q_len + k
    aw = synth.rand_field(f.field_id, 0x6D0001, la)
    bw = synth.rand_field(f.field_id, 0x6D0002, k + 1)
    q_ref, r_ref = ref_divide_stored(f, words_to_ints(aw), words_to_ints(bw))
    a = arena(4 * la + 4 * q_len + 5 * PAGE_WORDS)
    a0 = PAGE_WORDS + 1
    q0 = a0 + 4 * la + (-(a0 + 4 * la) % PAGE_WORDS) + PAGE_WORDS + 1
    ra = arena(2 * PAGE_WORDS)
    r0 = PAGE_WORDS + 1
    a[a0:a0 + 4 * la] = aw.reshape(-1)
    before = stats(L)
    lib.check(L.plk_poly_division(f.field_id, ptr(a[a0:]), la, ptr(bw), k + 1, ptr(a[q0:]), q_len, ptr(ra[r0:])))
    assert delta(L, before) == {"fresh": 2, "direct": 2, "staged": 1}
    assert np.array_equal(a[q0:q0 + 4 * q_len].reshape(-1, 4), ints_to_words(q_ref))
    assert np.array_equal(ra[r0:r0 + 4 * k].reshape(-1, 4), ints_to_words(r_ref))
    assert np.array_equal(a[a0:a0 + 4 * la].reshape(-1, 4), aw), "the dividend was changed"
    assert only_poison(a, (a0, a0 + 4 * la), (q0, q0 + 4 * q_len)) and only_poison(ra, (r0, r0 + 4 * k))


# ---- the staging buffer runs full ----
def test_staging_buffer_full(L):
    """plk_ntt_batch of 160 transforms of 32 KiB: 5 MiB of small pieces against a staging buffer of at most 4 MiB (PIN_CAP; it does
    not grow while pieces of it are in flight, so it may be as small as 256 KiB).  The uploads that no longer fit and, the buffer
    still being full, ALL the downloads fall through to direct copies."""
    log_n, batch = 10, 160
    pre = ol.FftPrecomputation(F, 1 << log_n)
    xs = synth.rand_field(F, 0x6E0001, batch << log_n).reshape(batch, -1)
    w = xs.shape[1]
    a = arena(batch * (w + 8) + 2 * PAGE_WORDS)
    o = arena(batch * (w + 8) + 2 * PAGE_WORDS)
    at = [PAGE_WORDS + 1 + b * (w + 8) for b in range(batch)]  # eight poisoned words between neighbours
    for b in range(batch):
        a[at[b]:at[b] + w] = xs[b]
    pi = (ctypes.c_void_p * batch)(*[a[i:].ctypes.data for i in at])
    po = (ctypes.c_void_p * batch)(*[o[i:].ctypes.data for i in at])
    before = stats(L)
    lib.check(L.plk_ntt_batch(F, log_n, 0, batch, pi, po))
    d = delta(L, before)
    assert set(d) == {"staged", "direct"} and d["staged"] + d["direct"] == 2 * batch
    assert 1 <= d["staged"] <= 128 and d["direct"] >= batch + 32, d
    for b in range(batch):
        assert np.array_equal(o[at[b]:at[b] + w].reshape(-1, 4), pre.fft_with_precomputation_power_of_2(xs[b].reshape(-1, 4))), b
        assert np.array_equal(a[at[b]:at[b] + w], xs[b])
    holes = [(i, i + w) for i in at]
    assert only_poison(a, *holes) and only_poison(o, *holes)


# ---- one thread, overlapping buffers in one batched call ----
def test_overlapping_inputs_of_one_batched_call(L):
    """plk_ntt_batch, batch 3, 2^15: in[1] starts in the middle of in[0], in[2] IS in[0]; the outputs are adjacent.  The second
    input extends this thread's own registration: the union path, with its device synchronisation in the middle of the call."""
    log_n = 15
    n = 1 << log_n
    A = synth.rand_field(F, 0x6F0001, 3 * n // 2)
    pre = ol.FftPrecomputation(F, n)
    want = [pre.fft_with_precomputation_power_of_2(A[:n]), pre.fft_with_precomputation_power_of_2(A[n // 2:])]
    want.append(want[0])
    a = arena(A.size + 2 * PAGE_WORDS)
    o = arena(3 * 4 * n + 2 * PAGE_WORDS)
    a0 = o0 = PAGE_WORDS + 1
    a[a0:a0 + A.size] = A.reshape(-1)
    ins = [a0, a0 + 4 * (n // 2), a0]
    pi = (ctypes.c_void_p * 3)(*[a[i:].ctypes.data for i in ins])
    po = (ctypes.c_void_p * 3)(*[o[o0 + b * 4 * n:].ctypes.data for b in range(3)])
    before = stats(L)
    lib.check(L.plk_ntt_batch(F, log_n, 0, 3, pi, po))
    # in[0] out[0] fresh, in[1] the union, out[1] fresh (adjacent is not overlapping), in[2] inside the union, out[2] fresh
    assert delta(L, before) == {"fresh": 4, "union": 1, "shared": 1, "direct": 6}
    for b in range(3):
        assert np.array_equal(o[o0 + b * 4 * n:o0 + (b + 1) * 4 * n].reshape(n, 4), want[b]), b
    assert np.array_equal(a[a0:a0 + A.size].reshape(A.shape), A), "the inputs were changed"
    assert only_poison(a, (a0, a0 + A.size)) and only_poison(o, (o0, o0 + 3 * 4 * n))
    assert stats(L)["released-last"] - before["released-last"] == 4  # the union once, at its last release


def test_in_place_batched_call(L):
    """plk_ntt_batch, batch 3, 2^15, out[b] == in[b] on three disjoint (adjacent) inputs: one registration per buffer."""
    log_n = 15
    n = 1 << log_n
    refs = [vec(F, log_n, 0x6B0000 + b) for b in range(3)]
    a = arena(3 * 4 * n + 2 * PAGE_WORDS)
    a0 = PAGE_WORDS + 1
    for b in range(3):
        a[a0 + b * 4 * n:a0 + (b + 1) * 4 * n] = refs[b][0].reshape(-1)
    p = (ctypes.c_void_p * 3)(*[a[a0 + b * 4 * n:].ctypes.data for b in range(3)])
    before = stats(L)
    lib.check(L.plk_ntt_batch(F, log_n, 0, 3, p, p))
    assert delta(L, before) == {"fresh": 3, "direct": 6}
    for b in range(3):
        assert np.array_equal(a[a0 + b * 4 * n:a0 + (b + 1) * 4 * n].reshape(n, 4), refs[b][1]), b
    assert only_poison(a, (a0, a0 + 3 * 4 * n))


# ---- threads (ctypes releases the GIL) ----
def run_threads(jobs):
    """every job on a thread of its own, started together; the jobs' return codes"""
    rcs = [None] * len(jobs)
    gate = threading.Barrier(len(jobs))

    def work(i):
        gate.wait()
        rcs[i] = jobs[i]()

    ts = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return rcs


ROUNDS = 20


def test_threads_share_one_input(L):
    """Eight threads transform the SAME 1 MiB input into adjacent slices of one arena, 20 rounds: with plk_ntt (nothing registered),
    then with plk_ntt_batch of the input twice (the input's registration is shared between the threads, released by the last one;
    the adjacent outputs are registrations of their own)."""
    log_n, T = 15, 8
    x, y = vec(F, log_n, 0x700001)
    w = x.size
    a = arena(w + 2 * PAGE_WORDS)
    a0 = PAGE_WORDS + 1
    a[a0:a0 + w] = x.reshape(-1)
    o = arena(2 * T * w + 2 * PAGE_WORDS)
    o0 = PAGE_WORDS + 1
    before = stats(L)
    for r in range(ROUNDS):
        o[:] = POISON
        rcs = run_threads([lambda t=t: L.plk_ntt(F, log_n, 0, ptr(a[a0:]), ptr(o[o0 + t * w:])) for t in range(T)])
        assert rcs == [lib.PLK_OK] * T, (r, rcs)
        assert np.array_equal(o[o0:o0 + T * w].reshape(T, -1, 4), np.broadcast_to(y, (T,) + y.shape)), r
        assert only_poison(o, (o0, o0 + T * w))
    assert delta(L, before) == {"direct": 2 * T * ROUNDS}
    before = stats(L)
    pi = (ctypes.c_void_p * 2)(a[a0:].ctypes.data, a[a0:].ctypes.data)
    pos = [(ctypes.c_void_p * 2)(o[o0 + 2 * t * w:].ctypes.data, o[o0 + (2 * t + 1) * w:].ctypes.data) for t in range(T)]
    for r in range(ROUNDS):
        o[:] = POISON
        rcs = run_threads([lambda t=t: L.plk_ntt_batch(F, log_n, 0, 2, pi, pos[t]) for t in range(T)])
        assert rcs == [lib.PLK_OK] * T, (r, rcs)
        assert np.array_equal(o[o0:o0 + 2 * T * w].reshape(2 * T, -1, 4), np.broadcast_to(y, (2 * T,) + y.shape)), r
        assert only_poison(o, (o0, o0 + 2 * T * w))
    d = delta(L, before)
    # per call: the input twice (fresh or shared), two outputs (fresh); nobody waits for anybody, nothing is refused
    assert d.pop("fresh") + d.pop("shared") == 4 * T * ROUNDS and d == {"direct": 4 * T * ROUNDS}
    assert np.array_equal(a[a0:a0 + w].reshape(x.shape), x) and only_poison(a, (a0, a0 + w))


def test_threads_nested_and_overlapping_inputs(L):
    """Two threads, 20 rounds each way: a 2^16 transform over A[0:2^16] beside a 2^15 one over A[2^15:2^16] (nested), and 2^15
    transforms over A[0:2^15] and A[2^14:2^14 + 2^15] (partly overlapping) - with plk_ntt, then with the overlapping pair as
    plk_ntt_batch of the input twice, where the second thread's request extends the first one's registration and has to wait for
    its release (or the other way round): milliseconds, never the two-second limit."""
    n15, n16 = 1 << 15, 1 << 16
    A = synth.rand_field(F, 0x710001, n16)
    p15, p16 = ol.FftPrecomputation(F, n15), ol.FftPrecomputation(F, n16)
    y_all, y_top = p16.fft_with_precomputation_power_of_2(A), p15.fft_with_precomputation_power_of_2(A[n15:])
    y_lo, y_mid = p15.fft_with_precomputation_power_of_2(A[:n15]), p15.fft_with_precomputation_power_of_2(A[n15 // 2:n15 // 2 + n15])
    a = arena(A.size + 2 * PAGE_WORDS)
    a0 = PAGE_WORDS + 1
    a[a0:a0 + A.size] = A.reshape(-1)
    o = arena(16 * n15 + 3 * PAGE_WORDS)  # the largest use: four 2^15 outputs of the batched pair
    o0 = PAGE_WORDS + 1
    o1 = o0 + 4 * n16
    assert o1 + 4 * n15 <= o.size and o0 + 16 * n15 <= o.size
    before = stats(L)
    for r in range(ROUNDS):
        o[:] = POISON
        rcs = run_threads([lambda: L.plk_ntt(F, 16, 0, ptr(a[a0:]), ptr(o[o0:])),
                           lambda: L.plk_ntt(F, 15, 0, ptr(a[a0 + 4 * n15:]), ptr(o[o1:]))])
        assert rcs == [lib.PLK_OK] * 2, (r, rcs)
        assert np.array_equal(o[o0:o1].reshape(n16, 4), y_all) and np.array_equal(o[o1:o1 + 4 * n15].reshape(n15, 4), y_top), r
        assert only_poison(o, (o0, o1 + 4 * n15))
        o[:] = POISON
        rcs = run_threads([lambda: L.plk_ntt(F, 15, 0, ptr(a[a0:]), ptr(o[o0:])),
                           lambda: L.plk_ntt(F, 15, 0, ptr(a[a0 + 4 * (n15 // 2):]), ptr(o[o0 + 4 * n15:]))])
        assert rcs == [lib.PLK_OK] * 2, (r, rcs)
        assert np.array_equal(o[o0:o0 + 4 * n15].reshape(n15, 4), y_lo) and np.array_equal(o[o0 + 4 * n15:o0 + 8 * n15].reshape(n15, 4), y_mid), r
        assert only_poison(o, (o0, o0 + 8 * n15))
    assert delta(L, before) == {"direct": 8 * ROUNDS}
    before = stats(L)
    starts = [a0, a0 + 4 * (n15 // 2)]
    pis = [(ctypes.c_void_p * 2)(a[s:].ctypes.data, a[s:].ctypes.data) for s in starts]
    pos = [(ctypes.c_void_p * 2)(o[o0 + 2 * t * 4 * n15:].ctypes.data, o[o0 + (2 * t + 1) * 4 * n15:].ctypes.data) for t in range(2)]
    for r in range(ROUNDS):
        o[:] = POISON
        rcs = run_threads([lambda t=t: L.plk_ntt_batch(F, 15, 0, 2, pis[t], pos[t]) for t in range(2)])
        assert rcs == [lib.PLK_OK] * 2, (r, rcs)
        got = o[o0:o0 + 16 * n15].reshape(4, n15, 4)
        assert np.array_equal(got[0], y_lo) and np.array_equal(got[1], y_lo) and np.array_equal(got[2], y_mid) and np.array_equal(got[3], y_mid), r
        assert only_poison(o, (o0, o0 + 16 * n15))
    d = delta(L, before)
    assert "gave-up" not in d and "register-failed" not in d and "union-failed" not in d and "bounced" not in d, d
    assert d["direct"] == 8 * ROUNDS and d["fresh"] + d["shared"] == 8 * ROUNDS, d
    assert np.array_equal(a[a0:a0 + A.size].reshape(A.shape), A) and only_poison(a, (a0, a0 + A.size))


def test_threads_share_one_scalar_vector(L, msm):
    """Four threads run plk_msm_execute on ONE context with the same scalar buffer, 20 rounds."""
    ctx, s, exp, ez = msm
    T = 4
    sa = arena(s.size + 2 * PAGE_WORDS)
    s0 = PAGE_WORDS + 1
    sa[s0:s0 + s.size] = s.reshape(-1)
    xy, zero = arena(T * 8 + 2 * PAGE_WORDS), arena(4096 + 64, np.uint8)
    x0, z0 = PAGE_WORDS + 1, 4096 + 3
    for r in range(ROUNDS):
        xy[:] = POISON
        zero[:] = 0xA5
        rcs = run_threads([lambda t=t: L.plk_msm_execute(ctx, ptr(sa[s0:]), 1 << 15, ptr(xy[x0 + 8 * t:]), ptr(zero[z0 + t:])) for t in range(T)])
        assert rcs == [lib.PLK_OK] * T, (r, rcs)
        assert np.array_equal(xy[x0:x0 + 8 * T].reshape(T, 2, 4), np.broadcast_to(exp, (T, 2, 4))), r
        assert list(zero[z0:z0 + T]) == [ez] * T
        assert only_poison(xy, (x0, x0 + 8 * T)) and only_poison(zero, (z0, z0 + T))
    assert np.array_equal(sa[s0:s0 + s.size].reshape(s.shape), s) and only_poison(sa, (s0, s0 + s.size))


# ---- memory the caller registered itself ----
def test_memory_the_caller_registered(L):
    """INTEGRATION.md's contract for a host pointer: any readable and writable host memory, PLK_OK, exact bits - also where the
    caller has registered a part of its arena with the runtime (hipHostRegister) for transfers of its own.  The runtime resolves a
    host pointer to the registered object it starts in and rejects a copy that runs past that object's end ("invalid argument");
    such a buffer is copied in chunks through pinned memory of the lane (host_lane.h: lane_h2d_bounced) - case (b) with plk_ntt.  In
    the batched call the library registers the buffer itself, which the runtime accepts, and the copies are direct.  Buffers (a) exactly the registered 1 MiB, (b) starting in its middle and running past its
    end, (c) 2 MiB containing it; each as the input and as the output of plk_ntt, and (b) in a batched call, which tries to register."""
    import torch
    rt = torch.cuda.cudart()
    code = lambda rc: int(getattr(rc, "value", rc))  # noqa: E731
    n15, n16 = 1 << 15, 1 << 16
    MIB_W = (1 << 20) // 8
    a = arena(6 * MIB_W)
    reg_lo = 2 * MIB_W  # the caller's registration: [2 MiB, 3 MiB) of the arena
    cases = {"a": (15, reg_lo), "b": (15, reg_lo + MIB_W // 2 + 1), "c": (16, reg_lo - MIB_W // 2 + 1)}
    plain = arena(4 * n16 + 2 * PAGE_WORDS)
    p0 = PAGE_WORDS + 1
    assert code(rt.cudaHostRegister(a[reg_lo:].ctypes.data, 1 << 20, 0)) == 0
    try:
        for name, (log_n, at) in sorted(cases.items()):
            x, y = vec(F, log_n, 0x720000 + log_n)
            w = x.size
            # the case's buffer as the input
            a[:] = POISON
            plain[:] = POISON
            a[at:at + w] = x.reshape(-1)
            before = stats(L)
            rc = L.plk_ntt(F, log_n, 0, ptr(a[at:]), ptr(plain[p0:]))
            print("caller-registered (%s) as input: rc %d %s %r" % (name, rc, L.plk_last_error() if rc or "bounced" in delta(L, before) else b"", delta(L, before)))
            assert rc == lib.PLK_OK, (name, L.plk_last_error())
            assert np.array_equal(plain[p0:p0 + w].reshape(y.shape), y), name
            assert ("bounced" in delta(L, before)) == (name == "b"), "the route of case (%s) changed" % name
            assert np.array_equal(a[at:at + w].reshape(x.shape), x) and only_poison(a, (at, at + w)) and only_poison(plain, (p0, p0 + w)), name
            # ... as the output
            a[:] = POISON
            plain[:] = POISON
            plain[p0:p0 + w] = x.reshape(-1)
            before = stats(L)
            rc = L.plk_ntt(F, log_n, 0, ptr(plain[p0:]), ptr(a[at:]))
            print("caller-registered (%s) as output: rc %d %s %r" % (name, rc, L.plk_last_error() if rc or "bounced" in delta(L, before) else b"", delta(L, before)))
            assert rc == lib.PLK_OK, (name, L.plk_last_error())
            assert np.array_equal(a[at:at + w].reshape(y.shape), y), name
            assert only_poison(a, (at, at + w)) and only_poison(plain, (p0, p0 + w)), name
        # (b) twice in one batched call, in place beside a plain buffer: the registry asks for a registration of its own
        x, y = vec(F, 15, 0x720000 + 15)
        w = x.size
        at = cases["b"][1]
        a[:] = POISON
        plain[:] = POISON
        a[at:at + w] = x.reshape(-1)
        plain[p0:p0 + w] = x.reshape(-1)
        p = (ctypes.c_void_p * 2)(a[at:].ctypes.data, plain[p0:].ctypes.data)
        before = stats(L)
        rc = L.plk_ntt_batch(F, 15, 0, 2, p, p)
        print("caller-registered (b) batched in place: rc %d %s %r" % (rc, L.plk_last_error() if rc or "bounced" in delta(L, before) else b"", delta(L, before)))
        assert rc == lib.PLK_OK, L.plk_last_error()
        assert np.array_equal(a[at:at + w].reshape(y.shape), y) and np.array_equal(plain[p0:p0 + w].reshape(y.shape), y)
        assert only_poison(a, (at, at + w)) and only_poison(plain, (p0, p0 + w))
    finally:
        assert code(rt.cudaHostUnregister(a[reg_lo:].ctypes.data)) == 0
