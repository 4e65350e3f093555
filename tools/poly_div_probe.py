"""Times the general polynomial division and the series inverse (polydiv_newton.hip) against the reference's own route composed from
plk_poly_mul_dev, and the two division routes side by side at the recurrence route's limit.

    python tools/poly_div_probe.py [--log-la 20] [--reps 9]

Everything runs on Tweedledee's scalar field, on one stream, timed with events: the median of --reps runs after two warm-up runs.
The yardstick is Polynomial::inv_mod_xn / polynomial_division (polynomial.rs:261-327) as written, driven from the host: three
Polynomial::mul per level at the reference's operand lengths, then the two products of the division.  Its additions, negations and
reversals are left out (in its favour); every plk_poly_mul_dev reads its operands' degrees back, as Polynomial::mul does."""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plonky_amd import api, device as dev, lib  # noqa: E402

FIELD = api.TWEEDLEDUM_BASE
P = 0x40000000000000000000000000000000038aa1276c3f59b9a14064e200000001


def rand_elems(rs, n):
    w = np.frombuffer(rs.bytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
    w[:, 3] &= np.uint64((1 << 61) - 1)  # below 2^253 < p: reduced words
    return dev.to_device(w)


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def mul(x, y, out):
    got = ctypes.c_size_t(0)
    lib.check(lib.load().plk_poly_mul_dev(FIELD, ctypes.c_void_p(x.data_ptr()), x.shape[0], ctypes.c_void_p(y.data_ptr()), y.shape[0],
                                          ctypes.c_void_p(out.data_ptr()), out.shape[0], ctypes.byref(got), dev._stream()))
    return got.value


def reference_inverse(h, n, work):
    """the launches of inv_mod_xn: per level a.mul(h0), a.mul(h1), a.mul(tmp) with len a = l, h0 = h[..l], h1 = h[l..]"""
    l = 1
    while l < n:
        a, h0, h1 = work[0][:l], h[:l], h[l:n]
        mul(a, h0, work[1])
        mul(a, h1, work[2])
        mul(a, work[1][:max(len(h1) + l - 1, 1)], work[3])
        l *= 2


def reference_division(a, b, work):
    m = a.shape[0] - b.shape[0] + 1
    reference_inverse(b[:m], m, work)
    mul(work[0][:m], a[:m], work[1])
    mul(work[1][:m], b, work[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-la", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    dev.init()
    la, rs = 1 << args.log_la, np.random.RandomState(1)
    print("device:", torch.cuda.get_device_name(0), "| field: Tweedledee scalar | la = n = 2^%d | median (min .. max) ms of %d runs" % (args.log_la, args.reps))
    a = rand_elems(rs, la)
    work = [rand_elems(rs, 4 * la) for _ in range(4)]
    q = torch.empty((la, 4), dtype=torch.int64, device="cuda")
    for k in (33, 1 << (args.log_la // 2), 1 << (args.log_la - 1)):
        b = rand_elems(rs, k + 1)
        rem = torch.empty((k, 4), dtype=torch.int64, device="cuda")
        new = timed(lambda: dev.polynomial_div_rem_dev(FIELD, a, b, out=q[:la - k], rem=rem), args.reps)
        ref = timed(lambda: reference_division(a, b, work), args.reps)
        print("div_rem k = %-7d  newton %8.3f (%.3f .. %.3f)   reference route over poly_mul %8.3f (%.3f .. %.3f)" % ((k,) + new + ref))
    h = rand_elems(rs, la)
    new = timed(lambda: dev.polynomial_inv_mod_xn_dev(FIELD, h, la, out=q), args.reps)
    ref = timed(lambda: reference_inverse(h, la, work), args.reps)
    print("inv_mod_xn n = 2^%-4d  newton %8.3f (%.3f .. %.3f)   reference route over poly_mul %8.3f (%.3f .. %.3f)" % ((args.log_la,) + new + ref))
    k = 32
    b = rand_elems(rs, k + 1)
    bh = dev.to_host(b)
    rem = torch.empty((k, 4), dtype=torch.int64, device="cuda")
    rec = timed(lambda: dev.polynomial_division_dev(FIELD, a, bh, out=q[:la - k], rem=rem), args.reps)
    new = timed(lambda: dev.polynomial_div_rem_dev(FIELD, a, b, out=q[:la - k], rem=rem), args.reps)
    print("routes at k = 32     recurrence %8.3f (%.3f .. %.3f)   newton %8.3f (%.3f .. %.3f)" % (rec + new))


if __name__ == "__main__":
    main()
