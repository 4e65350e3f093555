"""Timing of the two Plookup kernels (plookup.hip) beside the permutation Z of the same row count, in one process.

    python tools/plookup_probe.py [--field 1] [--out profiles/r10_plookup.txt]

For N = 2^16, 2^18, 2^20: plk_plookup_grand_product_dev, plk_plonk_permutation_z_dev (stride 1, log_degree = log N) and
plk_plookup_vanishing_points_dev (4N points), each warmed (the tables are built by the first call), then timed with HIP events over
REPEATS windows of CALLS back-to-back calls; median and spread per call.  Bytes are by count (what a row / point reads and writes
once), the rates stand beside the ceilings plk_bench_ceilings measures in this process.
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from plonky_amd import device as dev, lib, synth  # noqa: E402

REPEATS, CALLS = 9, 8
MARKER = "---- measured (tools/plookup_probe.py) ----"
ROW_BYTES = 4 * 32 + 32        # f, t, s, s at n + j read once a row (the neighbours are shared), one value written twice over (rows, fix-up: + 64 below)
POINT_BYTES = 9 * 32 + 2 * 32 + 32   # nine row elements, two L_0 entries, one output


def timed(fn):
    """milliseconds per call: median and (min, max) over REPEATS windows of CALLS calls between two events"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / CALLS)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "r10_plookup.txt"))
    args = ap.parse_args()
    dev.init(0)
    fid = args.field
    lines = ["plookup_probe: field %d, %s, %d windows of %d calls, ms per call: median (min .. max)" % (fid, torch.cuda.get_device_name(0), REPEATS, CALLS)]
    ceil = (ctypes.c_double * 8)()
    lib.check(lib.load().plk_bench_ceilings(ceil, 8))
    lines.append("plk_bench_ceilings: %.1f G v_mad_u64_u32 lane-ops/s, %.2f G 9-limb Montgomery products/s (4 waves per SIMD)" % (ceil[0], ceil[1]))
    sc = synth.rand_field(fid, 5, 9)
    for log_n in (16, 18, 20):
        n = 1 << log_n
        f, t = (dev.to_device(synth.rand_field(fid, 10 + i, n)) for i in range(2))
        s = dev.to_device(synth.rand_field(fid, 12, 2 * n - 1))
        wires, sigma = (dev.to_device(synth.rand_field(fid, 20 + i, 6 * n).reshape(6, n, 4)) for i in range(2))
        out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        gp = timed(lambda: dev.plookup_grand_polynomial_dev(fid, log_n, f, t, s, sc[0], sc[1], out=out))
        z = timed(lambda: dev.permutation_polynomial_dev(fid, log_n, wires, sigma, sc[2:8], sc[0], sc[1], sigma_stride=1, out=out))
        del wires, sigma
        vals = dev.to_device(synth.rand_field(fid, 30, 5 * 4 * n).reshape(5, 4 * n, 4))
        pout = torch.empty((4 * n, 4), dtype=torch.int64, device="cuda")
        pt = timed(lambda: dev.plookup_vanishing_values_dev(fid, log_n, vals, sc[8], sc[0], sc[1], out=pout))
        gp_bytes, pt_bytes = n * (ROW_BYTES + 64), 4 * n * POINT_BYTES
        lines.append("N = 2^%d" % log_n)
        lines.append("  grand product     %8.4f (%.4f .. %.4f)  %6.1f Mrow/s  %6.1f GB/s by count" % (*gp, n / gp[0] / 1e3, gp_bytes / gp[0] / 1e6))
        lines.append("    products by count: 11 a row + a quarter of an inversion -> %.2f G products/s; a point: 12 products + 3 shared reductions -> %.2f G products/s"
                     % (11 * n / gp[0] / 1e6, 12 * 4 * n / pt[0] / 1e6))
        lines.append("  permutation Z     %8.4f (%.4f .. %.4f)  %6.1f Mrow/s  grand product / Z = %.3f" % (*z, n / z[0] / 1e3, gp[0] / z[0]))
        lines.append("  vanishing points  %8.4f (%.4f .. %.4f)  %6.1f Mpoint/s  %d bytes by count  %6.1f GB/s" % (*pt, 4 * n / pt[0] / 1e3, pt_bytes, pt_bytes / pt[0] / 1e6))
        del vals, pout, f, t, s
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        head = ""  # the resource report at the top of the file is kept: everything above the marker
        if os.path.exists(args.out):
            head = open(args.out).read().split(MARKER)[0]
        with open(args.out, "w") as fh:
            fh.write(head + MARKER + "\n" + text + "\n")


if __name__ == "__main__":
    main()
