"""Timing of the opening step (opening.hip) against the only device route the library offered before it, in one process:

  evaluations   eval_polys_dev (30 polynomials, 3 points)     vs  3 uploaded power vectors + 90 inner_product_dev calls
  reduction     reduce_polynomials_dev                        vs  29 chained fold_slices_dev calls
  halo_b        build_halo_b_dev                              vs  3 uploaded power vectors + 2 fold_slices_dev calls

Warmed, old and new alternating, every window at least half a second, REPEATS windows each; prints median and spread, the byte and
product counts of the new kernels and the ceilings plk_bench_ceilings measures in this process.

    python tools/opening_bench.py [--log-n 20] [--field 1] [--once]     (--once: one call of each new entry, for a profiler)
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from plonky_amd import device as dev, lib, synth  # noqa: E402

REPEATS = 7


def window(fn, min_seconds=0.5):
    """seconds per call over a window of at least min_seconds"""
    fn()
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        if calls % 4 == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= min_seconds:
                break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--field", type=int, default=1)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    dev.init(0)
    fid, n = args.field, 1 << args.log_n
    p = synth.MODULI[fid]
    polys = [dev.to_device(synth.rand_field(fid, 100 + i, n)) for i in range(30)]
    points = synth.rand_field(fid, 7, 3)
    scalars = synth.rand_field(fid, 8, 30)
    v = synth.rand_field(fid, 9, 1)[0]
    one = synth.mont(fid, 1)

    def new_eval():
        return dev.eval_polys_dev(fid, polys, points)

    def new_reduce():
        return dev.reduce_polynomials_dev(fid, polys, scalars, n)

    def new_b():
        return dev.build_halo_b_dev(fid, points, v, n)

    if args.once:
        for fn in (new_eval, new_reduce, new_b, new_eval, new_reduce, new_b):
            fn()
        torch.cuda.synchronize()
        print("ran each new entry twice")
        return

    # the parent's route needs the power vectors on the device: made on the host (as the reference does), uploaded once, not timed
    def host_powers(x_limbs):
        x = synth.from_mont(fid, x_limbs)
        cur, vals = synth.to_int(one), []
        for _ in range(n):
            vals.append(cur.to_bytes(32, "little"))
            cur = cur * x % p
        return np.frombuffer(b"".join(vals), dtype=np.uint64).reshape(n, 4).copy()
    t0 = time.perf_counter()
    pw = [dev.to_device(host_powers(points[k])) for k in range(3)]
    print("host powers + upload (not part of any timing below): %.1f s" % (time.perf_counter() - t0))
    v_i = synth.from_mont(fid, v)
    v2 = synth.mont(fid, v_i * v_i % p)

    def old_eval():
        return [dev.inner_product_dev(fid, c, pw[k]) for k in range(3) for c in polys]

    def old_reduce():
        acc = dev.fold_slices_dev(fid, polys[0], polys[1], scalars[0], scalars[1])
        for i in range(2, 30):
            acc = dev.fold_slices_dev(fid, acc, polys[i], one, scalars[i])
        return acc

    def old_b():
        return dev.fold_slices_dev(fid, dev.fold_slices_dev(fid, pw[0], pw[1], one, v), pw[2], one, v2)

    # the routes agree before anything is timed
    assert torch.equal(torch.cat(old_eval()).reshape(3, 30, 4), new_eval())
    assert torch.equal(old_reduce(), new_reduce())
    assert torch.equal(old_b(), new_b())

    steps = [("evaluations", old_eval, new_eval), ("reduction", old_reduce, new_reduce), ("halo_b", old_b, new_b)]
    res = {name: ([], []) for name, _, _ in steps}
    for _ in range(REPEATS):
        for name, old, new in steps:  # alternating old and new
            res[name][0].append(window(old))
            res[name][1].append(window(new))
    print("n = 2^%d, field %d, 30 polynomials, 3 points; ms per call: median [min .. max] of %d windows >= 0.5 s" % (args.log_n, fid, REPEATS))
    tot_old = tot_new = 0.0
    slower = []
    for name, _, _ in steps:
        o, w = np.array(res[name][0]) * 1e3, np.array(res[name][1]) * 1e3
        tot_old += np.median(o)
        tot_new += np.median(w)
        if not w.max() < o.min():  # the gain must exceed the run-to-run spread: every new window below every old one
            slower.append(name)
        print("%-12s old %8.3f [%8.3f .. %8.3f]   new %8.3f [%8.3f .. %8.3f]   x%.1f" % (name, np.median(o), o.min(), o.max(), np.median(w), w.min(), w.max(),
                                                                                     np.median(o) / np.median(w)))
    print("%-12s old %8.3f                          new %8.3f                          x%.1f" % ("together", tot_old, tot_new, tot_old / tot_new))
    ceil = (ctypes.c_double * 5)()
    lib.check(lib.load().plk_bench_ceilings(ceil, 5))
    print("plk_bench_ceilings: v_mad_u64_u32 %.0f G/s, 9-limb Montgomery product %.1f G/s" % (ceil[0], ceil[1]))
    ev, rd, hb = (np.median(res[k][1]) for k in ("evaluations", "reduction", "halo_b"))
    print("evaluations: %.0f MiB read, %.1f M coefficient-point products (81 multiplier instructions each, one reduction per 6)  -> %.2f TB/s, %.1f G products/s"
          % (30 * n * 32 / 2**20, 90 * n / 1e6, 30 * n * 32 / ev / 1e12, 90 * n / ev / 1e9))
    print("reduction:   %.0f MiB read + %.0f MiB written, %.1f M products -> %.2f TB/s, %.1f G products/s"
          % (30 * n * 32 / 2**20, n * 32 / 2**20, 30 * n / 1e6, 31 * n * 32 / rd / 1e12, 30 * n / rd / 1e9))
    print("halo_b:      %.0f MiB written, %.1f M products -> %.2f TB/s, %.1f G products/s" % (n * 32 / 2**20, 3 * n / 1e6, n * 32 / hb / 1e12, 3 * n / hb / 1e9))
    # which bound holds: the share of the HBM peak against the share of the product ceiling measured above (whole call, launches included)
    HBM_PEAK = 8.0e12  # bytes/s, MI355X
    for name, nbytes, prods, sec in (("evaluations", 30 * n * 32, 90 * n, ev), ("reduction", 31 * n * 32, 30 * n, rd), ("halo_b", n * 32, 3 * n, hb)):
        mem, mul = nbytes / sec / HBM_PEAK, prods / sec / (ceil[1] * 1e9)
        print("%-12s %4.1f %% of the HBM peak (8 TB/s), %4.1f %% of the product ceiling: nearer the %s bound" % (name, 100 * mem, 100 * mul, "HBM" if mem > mul else "multiplier"))
    if slower:
        print("NOT FASTER than the earlier route by more than the spread: %s" % ", ".join(slower))
        sys.exit(1)


if __name__ == "__main__":
    main()
