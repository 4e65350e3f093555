"""Timing of the per-element scalar multiplications on the device (scalar_mul.hip).

    python tools/scalar_mul_probe.py [curve] [log_count] [--out FILE]

(FILE: profiles/scalar_mul.txt for Tweedledee, profiles/scalar_mul_<curve>.txt otherwise; one file per run, written whole.)

plk_curve_scalar_mul_dev, plk_halo_n_mul_dev (128 bits) and plk_halo_n_dev at 2^16 and 2^20 elements (or 2^log_count alone) on `curve`
(default 0, Tweedledee; the halo entries are skipped on BLS12-377): warmed, timed with HIP events over REPEATS windows, median and spread
per call.  Beside them plk_curve_fold_pairs_dev over the same number of outputs - the nearest older kernel: two SHARED scalars per output -
and plk_bench_ceilings out[0] (v_mad_u64_u32 lane-operations per second) from the same process, with the fraction of that issue rate
the executed field products come to (DESIGN.md counts them: 9 per doubling, 10 per mixed addition, 126 / 294 multiply-adds per product).
One process, ended by an alarm after LIMIT seconds."""
import argparse
import ctypes
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plonky_amd import device as dev, lib, synth  # noqa: E402
from plonky_amd.selfcheck import GENERATORS, _mul  # noqa: E402

REPEATS = 7
LIMIT = 600
NAMES = {0: "Tweedledee", 1: "Tweedledum", 2: "Bls12377", 3: "Pallas", 4: "Vesta"}
BASE_FIELD = {0: 0, 1: 1, 2: 3, 3: 4, 4: 5}
SCALAR_FIELD = {0: 1, 1: 0, 2: 2, 3: 5, 4: 4}
DBL, MADD = 9, 10   # field products of xyzzz_dbl and xyzzz_madd (ecz.cuh)


def products(curve):
    """field products a wave EXECUTES per element (a masked addition still issues), chain only"""
    if curve == 2:
        return {"scalar_mul": 128 * (2 * DBL + MADD)}
    return {"scalar_mul": 130 * (DBL + MADD), "halo_n_mul": 64 * (DBL + MADD)}  # fold_pairs skips its empty columns grid-wide: its count depends on the two scalars


def timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("curve", nargs="?", type=int, default=0)
    ap.add_argument("log_count", nargs="?", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    signal.alarm(LIMIT)
    curve = args.curve
    if curve not in GENERATORS:
        sys.exit("curve %d: selfcheck.GENERATORS has a generator for %s only" % (curve, sorted(GENERATORS)))
    dev.init(0)
    ceil = (ctypes.c_double * 8)()
    lib.check(lib.load().plk_bench_ceilings(ceil, 8))
    mads = 294 if curve == 2 else 126
    if args.out is None:
        args.out = os.path.join("profiles", "scalar_mul.txt" if curve == 0 else "scalar_mul_%s.txt" % NAMES[curve].lower())
    prop = torch.cuda.get_device_properties(0)
    lines = ["scalar_mul_probe: %s (%s, %d compute units), %s, %d windows, ms per call: median (min .. max)"
             % (torch.cuda.get_device_name(0), getattr(prop, "gcnArchName", "?"), prop.multi_processor_count, NAMES[curve], REPEATS),
             "plk_bench_ceilings out[0]: %.1f G v_mad_u64_u32 lane-operations/s; %d per field product" % (ceil[0], mads)]
    prod = products(curve)

    def report(name, n, ms, key):
        tail = ""
        if key in prod:
            rate = prod[key] * mads * n / ms[0] / 1e6
            tail = "   %5d products each   %6.1f G mad/s   %3.0f%% of the issue rate" % (prod[key], rate, 100 * rate / ceil[0])
        lines.append("%-34s %9.3f (%9.3f .. %9.3f)   %8.2f M elements/s%s" % (name, ms[0], ms[1], ms[2], n / ms[0] / 1e3, tail))

    bf, sf = BASE_FIELD[curve], SCALAR_FIELD[curve]
    p = synth.MODULI[bf]
    G = GENERATORS[curve]
    D = _mul(p, 987654321, G)
    import numpy as np
    pt = lambda P: np.stack([synth.mont(bf, P[0]), synth.mont(bf, P[1])])
    for log_n in ([args.log_count] if args.log_count is not None else [16, 20]):
        n = 1 << log_n
        calls = 4 if log_n <= 16 else 1
        pts = dev.gen_bases_dev(curve, n, pt(G), pt(D))
        sc = dev.to_device(synth.rand_field(sf, 5 + log_n, n))
        out, oz = torch.empty_like(pts), torch.empty(n, dtype=torch.uint8, device="cuda")
        report("scalar_mul 2^%d" % log_n, n, timed(lambda: dev.scalar_mul_dev(curve, sc, pts, out=out, out_zero=oz), calls), "scalar_mul")
        report("scalar_mul 2^%d, one point" % log_n, n, timed(lambda: dev.scalar_mul_dev(curve, sc, pts[:1], out=out, out_zero=oz), calls), "scalar_mul")
        if curve != 2:
            report("halo_n_mul (128 bits) 2^%d" % log_n, n, timed(lambda: dev.halo_n_mul_dev(curve, sc, pts, out=out, out_zero=oz), calls), "halo_n_mul")
            so = torch.empty_like(sc)
            report("halo_n (128 bits) 2^%d" % log_n, n, timed(lambda: dev.halo_n_dev(curve, sc, out=so), calls), "halo_n")
        hi = dev.gen_bases_dev(curve, n, pt(D), pt(G))
        two = synth.rand_field(sf, 99, 2)
        report("fold_pairs (2 shared scalars) 2^%d" % log_n, n, timed(lambda: dev.fold_generators_dev(curve, pts, hi, two[0], two[1]), calls), "fold_pairs")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
