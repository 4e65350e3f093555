"""GPU: the three host-pointer entries that drive the lane through LaneCall like every other one - plk_msm_precompute_ex,
plk_halo_begin, plk_ntt_precompute_table (host_lane.h).  A call the device-side implementation refuses AFTER the wrapper has
enqueued its uploads is an ordinary error return; what it must leave behind: the code and text the library returned before the
entries were moved (tests/golden/capi_device_refusals.json), no word of the caller's memory touched, nothing registered, and a
lane whose next call is exact.  16 points are staged through the lane's pinned buffer, 2^11 (128 KiB) are copied directly."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from plonky_amd import lib, synth
from tests.test_gpu_host_buffers import F, L, PAGE_WORDS, arena, delta, only_poison, ptr, stats, vec  # noqa: F401  (L: the fixture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_device_refusals.json")
CURVE = 0  # Tweedledee: 4-limb coordinates and scalars


def refused_call(L, entry, n):
    """the call; returns (code, text, [(arena, first, end, contents)])"""
    def placed(words, seed, dtype=np.uint64):
        a = arena(words + 2 * PAGE_WORDS, dtype)
        x = synth.rand_field(0, seed, (words + 3) // 4).reshape(-1)[:words]
        if dtype == np.uint8:
            x = (x & 1).astype(np.uint8)
        a[PAGE_WORDS + 1:PAGE_WORDS + 1 + words] = x
        return (a, PAGE_WORDS + 1, PAGE_WORDS + 1 + words, x)
    at = lambda b: ptr(b[0][b[1]:])  # noqa: E731
    if entry == "plk_msm_precompute_ex":
        bufs = [placed(8 * n, 0x1A0E01), placed(n, 0x1A0E02, np.uint8)]
        rc = L.plk_msm_precompute_ex(CURVE, n, at(bufs[0]), at(bufs[1]), 0, 0, None)  # no out_ctx: only msm_precompute_dev_impl looks
    else:
        bufs = [placed(4 * n, 0x1A0E03), placed(4 * n, 0x1A0E04), placed(8 * n, 0x1A0E05), placed(n, 0x1A0E06, np.uint8)]
        out = ctypes.c_void_p()
        # no Pedersen H: only halo_begin_dev_impl looks
        rc = L.plk_halo_begin(CURVE, n, at(bufs[0]), at(bufs[1]), at(bufs[2]), at(bufs[3]), None, at(bufs[2]), 0, ctypes.byref(out))
        assert not out.value
    return rc, L.plk_last_error().decode(), bufs


@pytest.mark.parametrize("n,route", [(16, "staged"), (1 << 11, "direct")], ids=["16", "2^11"])
@pytest.mark.parametrize("entry", ["plk_msm_precompute_ex", "plk_halo_begin"])
def test_refused_after_the_uploads(L, entry, n, route):
    x, y = vec(F, 10, 0x6A0000 + 10)
    before = stats(L)
    rc, text, bufs = refused_call(L, entry, n)
    moved = delta(L, before)
    print(entry, n, rc, text, moved)
    assert [rc, text] == json.load(open(GOLDEN))["%s:%d" % (entry, n)]
    assert set(moved) <= {"staged", "direct"} and route in moved, moved  # the uploads were enqueued; nothing was registered
    for a, lo, hi, contents in bufs:
        assert np.array_equal(a[lo:hi], contents) and only_poison(a, (lo, hi))
    out = np.empty_like(y)
    lib.check(L.plk_ntt(F, 10, 0, ptr(x), ptr(out)))  # the same thread, the same lane, straight afterwards
    assert np.array_equal(out, y)


@pytest.mark.parametrize("log_n", [3, 11])
def test_ntt_precompute_table_matches_the_device_form(L, log_n):
    import torch
    words = ((2 << log_n) - 1) * 4
    d = torch.zeros(words, dtype=torch.int64, device="cuda")
    lib.check(L.plk_ntt_precompute_table_dev(F, log_n, d.data_ptr(), None))
    torch.cuda.synchronize()
    want = d.cpu().numpy().view(np.uint64)
    a = arena(words + 2 * PAGE_WORDS)
    before = stats(L)
    lib.check(L.plk_ntt_precompute_table(F, log_n, ptr(a[PAGE_WORDS + 1:])))
    assert set(delta(L, before)) == {"staged" if words * 8 < (64 << 10) else "direct"}
    assert np.array_equal(a[PAGE_WORDS + 1:PAGE_WORDS + 1 + words], want) and want.any()
    assert only_poison(a, (PAGE_WORDS + 1, PAGE_WORDS + 1 + words))
