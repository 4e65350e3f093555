"""Timing of the low-degree polynomial division (polydiv.hip) at la = 2^20, k in {1, 2, 4, 8, 32}, against the reference's own route
(polynomial.rs:299-327) as the library could run it on the device before: inv_mod_xn by Newton's iteration (polynomial.rs:262-294) and
the two closing products, written here over poly_mul_dev (scalar multiples and sums through reduce_polynomials_dev, reversal by
torch.flip), and against the ceilings plk_bench_ceilings measures in this process.  The count of the new entry is 2 la k' field
products (k' = next power of two >= k) plus the scan; a is read twice and q written once.

    python tools/poly_division_bench.py [--log-n 20] [--field 1] [--skip-newton]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from plonky_amd import api, device as dev, lib, synth  # noqa: E402

REPEATS = 5


def window(fn, min_seconds=0.3):
    """seconds per call over a window of at least min_seconds"""
    fn()
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= min_seconds:
            break
    return (time.perf_counter() - t0) / calls


def newton_division(F, a, b_host, one, minus_one):
    """polynomial_division by the reference's algorithm; a: (la, 4) device, b_host: (k + 1, 4) host, lead != 0 -> (q, r) on the device"""
    la, k = a.shape[0], b_host.shape[0] - 1
    m = la - k  # a_degree - b_degree + 1 quotient coefficients
    h = torch.zeros((max(m, 2), 4), dtype=torch.int64, device="cuda")
    h[: k + 1] = dev.to_device(b_host[::-1].copy())  # rev(b)
    inv = dev.to_device(api.field_op(F, "inverse", b_host[k:k + 1]))  # 1 / rev_b[0]
    length = 1
    while length < m:  # inv_mod_xn: a <- a | (-a (a h[:2l])[l:2l])[:l]
        e = dev.poly_mul_dev(F, inv, h[: 2 * length].contiguous())[length: 2 * length].contiguous()
        neg = dev.reduce_polynomials_dev(F, [e], minus_one, e.shape[0])
        nb = dev.poly_mul_dev(F, inv, neg)[:length]
        inv = torch.cat([inv, nb]).contiguous()
        length *= 2
    inv = inv[:m].contiguous()
    rev_a = torch.flip(a, dims=[0])[:m].contiguous()
    q = torch.flip(dev.poly_mul_dev(F, inv, rev_a)[:m], dims=[0]).contiguous()
    qb = dev.poly_mul_dev(F, q, dev.to_device(b_host))[:la].contiguous()
    r = dev.reduce_polynomials_dev(F, [a, qb], np.concatenate([one, minus_one]), la)
    return q, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--field", type=int, default=1)
    ap.add_argument("--skip-newton", action="store_true")
    args = ap.parse_args()
    F, la = args.field, 1 << args.log_n
    dev.init()
    a = dev.to_device(synth.rand_field(F, 1, la))
    one = np.array(synth.mont(F, 1), dtype=np.uint64).reshape(1, 4)
    minus_one = api.field_op(F, "neg", one)
    ceil = (ctypes.c_double * 5)()
    lib.check(lib.load().plk_bench_ceilings(ceil, 5))
    print("plk_bench_ceilings: v_mad_u64_u32 %.0f G/s, 9-limb Montgomery product %.1f G/s" % (ceil[0], ceil[1]))
    q_out = torch.empty((la, 4), dtype=torch.int64, device="cuda")
    for k in (1, 2, 4, 8, 32):
        b = api.polynomial_from_roots(F, synth.rand_field(F, 40 + k, k))
        rem = torch.empty((k, 4), dtype=torch.int64, device="cuda")
        new = np.array([window(lambda: dev.polynomial_division_dev(F, a, b, q_len=la, out=q_out, rem=rem)) for _ in range(REPEATS)]) * 1e3
        kp = 1 << (k - 1).bit_length()
        prods = 2 * la * kp
        line = "la = 2^%d k = %2d: division %8.3f ms [%8.3f .. %8.3f]   2 la k' = %.1f M products -> %.2f G products/s (%.0f %% of the product ceiling), %.0f MiB moved" % (
            args.log_n, k, np.median(new), new.min(), new.max(), prods / 1e6, prods / np.median(new) / 1e6, 100 * prods / (np.median(new) * 1e-3) / (ceil[1] * 1e9),
            3 * la * 32 / 2**20)
        if not args.skip_newton:
            q_ref, r_ref = newton_division(F, a, b, one, minus_one)
            same = torch.equal(q_ref, q_out[: la - k]) and torch.equal(r_ref[:k], rem) and not bool(r_ref[k:].any())
            old = np.array([window(lambda: newton_division(F, a, b, one, minus_one)) for _ in range(3)]) * 1e3
            line += "   Newton route over poly_mul_dev %8.3f ms [%8.3f .. %8.3f] x%.1f, same words: %s" % (np.median(old), old.min(), old.max(), np.median(old) / np.median(new), same)
        print(line)


if __name__ == "__main__":
    main()
