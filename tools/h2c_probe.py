"""Timing of the BLAKE3 hash to the curve (hash_to_curve.hip): rounds over a compacted work list against one lane per seed.

    python tools/h2c_probe.py [--out profiles/h2c.txt]

plk_hash_to_curve_dev for 2^14, 2^17 and 2^20 seeds on Tweedledee and 2^20 on BLS12-377, warmed, timed with HIP events over REPEATS
windows; median and spread per call.  The same in a child process with PLK_H2C_NAIVE=1 (knobs are read once): the A/B.  Then, on
Tweedledee at 2^20:
  tries per generator   the try i at which each seed settled, found through the public entries alone: the x of the point equals the x
                        of plk_blake_field(i, seed) at exactly that i
  dense run             plk_hash_field_to_curve_dev over seeds that all settle at try 0 (2^20 of them, the loop form of the child
                        process: one try per lane, no list): the cost of a try
  rejection overhead    the full run / (tries x cost of a try)
  products per try      of a residue, counted from the exponent of the square root and the mean number of Tonelli-Shanks steps,
                        beside the product ceiling plk_bench_ceilings measures in this process
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plonky_amd import api, device as dev, lib, synth  # noqa: E402

REPEATS = 7
MARKER = "---- measured (tools/h2c_probe.py) ----"
CASES = ((0, 14), (0, 17), (0, 20), (2, 20))
NAMES = {0: "Tweedledee", 2: "BLS12-377"}


def timed(fn, calls):
    """milliseconds per call: median and (min, max) over REPEATS windows of `calls` calls between two events"""
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


def time_cases(dense_seeds=None):
    out = {}
    for curve, log_n in CASES:
        n = 1 << log_n
        buf = torch.empty((n, 2, 6 if curve == 2 else 4), dtype=torch.int64, device="cuda")
        out["%d/%d" % (curve, log_n)] = timed(lambda: dev.hash_to_curve_dev(curve, n, out=buf), 8 if log_n < 20 else 2)
    if dense_seeds is not None:
        d = dev.to_device(dense_seeds)
        buf = torch.empty((d.shape[0], 2, 4), dtype=torch.int64, device="cuda")
        out["dense"] = timed(lambda: dev.hash_to_curve_dev(0, d.shape[0], seeds=d, out=buf), 2)
    return out


def settle_tries(curve, n):
    """the try at which each of the seeds 0 .. n-1 settles, and the seeds in Montgomery form"""
    f = api.CURVE_BASE_FIELD[curve]
    canon = np.zeros((n, 4), dtype=np.uint64)
    canon[:, 0] = np.arange(n, dtype=np.uint64)
    seeds = api.field_op(f, "from_canonical", canon)
    x = api.blake_hash_usize_to_curve(curve, 0, n)[:, 0, :]
    tries = np.full(n, -1, dtype=np.int64)
    open_idx = np.arange(n)
    for i in range(256):
        if open_idx.size == 0:
            break
        xi, _ = api.blake_field(f, i, seeds[open_idx])
        hit = (xi == x[open_idx]).all(axis=1)
        tries[open_idx[hit]] = i
        open_idx = open_idx[~hit]
    assert open_idx.size == 0
    return tries, seeds


def products_per_try(field, steps_mean):
    """field products of one try: x^3 + B (2), the power a^((T-1)/2) (one squaring per bit below the top, one product per set bit
    below the top), x = w a and b = x w (2), and per Tonelli-Shanks step the squarings that find k, z = w^2, b z and x w"""
    p, adic = synth.MODULI[field], {0: 34, 3: 46}[field]
    e = (p - 1) >> (adic + 1)
    return 2 + (e.bit_length() - 1) + (bin(e).count("1") - 1) + 2 + steps_mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "h2c.txt"))
    ap.add_argument("--child", help="internal: time the cases (and the dense seeds of this .npy file) and print one JSON line")
    args = ap.parse_args()
    dev.init(0)
    if args.child:
        dense = np.load(args.child) if args.child != "-" else None
        print("H2C_CHILD " + json.dumps(time_cases(dense)))
        return
    lines = ["h2c_probe: %s, %d windows, ms per call: median (min .. max)" % (torch.cuda.get_device_name(0), REPEATS)]
    ceil = (ctypes.c_double * 8)()
    lib.check(lib.load().plk_bench_ceilings(ceil, 8))
    lines.append("plk_bench_ceilings: %.1f G v_mad_u64_u32 lane-ops/s; Montgomery products at 4 waves per SIMD: %.2f G/s (Tweedledee), %.2f G/s (BLS12-377)"
                 % (ceil[0], ceil[1], ceil[2]))
    n = 1 << 20
    tries, seeds = settle_tries(0, n)
    per_gen = float((tries + 1).mean())
    first = seeds[tries == 0]
    dense = np.concatenate([first] * (n // first.shape[0] + 1))[:n]
    dense_path = os.path.join(tempfile.mkdtemp(prefix="h2c_probe_"), "dense_seeds.npy")
    np.save(dense_path, dense)
    rounds = time_cases(dense)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", dense_path], capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, PLK_H2C_NAIVE="1"), cwd=ROOT)
    os.remove(dense_path)
    os.rmdir(os.path.dirname(dense_path))
    assert child.returncode == 0, (child.stdout + child.stderr)[-3000:]
    loop = json.loads([ln for ln in child.stdout.splitlines() if ln.startswith("H2C_CHILD ")][0][len("H2C_CHILD "):])
    lines.append("%-26s %-34s %-34s %s" % ("case", "rounds over a compacted list", "one lane per seed (PLK_H2C_NAIVE)", "loop / rounds"))
    for curve, log_n in CASES:
        key = "%d/%d" % (curve, log_n)
        r, l = rounds[key], loop[key]
        lines.append("%-26s %8.3f (%8.3f .. %8.3f)       %8.3f (%8.3f .. %8.3f)       x%.2f   %.1f M generators/s"
                     % ("%s 2^%d" % (NAMES[curve], log_n), r[0], r[1], r[2], l[0], l[1], l[2], l[0] / r[0], (1 << log_n) / r[0] / 1e3))
    lines.append("Tweedledee, seeds 0 .. 2^20 - 1: %.4f tries per generator, the slowest seed settles at try %d; seeds that settle at try 0: %d"
                 % (per_gen, int(tries.max()), first.shape[0]))
    dense_ms = loop["dense"][0]
    lines.append("dense run (2^20 seeds that settle at try 0, one try per lane): %.3f ms loop form (%.3f .. %.3f), %.3f ms through the rounds"
                 % (dense_ms, loop["dense"][1], loop["dense"][2], rounds["dense"][0]))
    full = rounds["0/20"][0]
    lines.append("rejection overhead: full run %.3f ms / (%.4f tries x %.3f ms) = %.2f   (loop form: %.2f)"
                 % (full, per_gen, dense_ms, full / (per_gen * dense_ms), loop["0/20"][0] / (per_gen * dense_ms)))
    # a residue's b = a^T is a uniform element of the subgroup of order 2^(adicity - 1): one Tonelli-Shanks step per set bit of its
    # exponent, (adicity - 1) / 2 on average, each with adicity / 2 squarings on average to find k and three products
    prods = products_per_try(0, (33 / 2) * (34 / 2 + 3))
    lines.append("about %.0f field products per try of a residue (counted: x^3 + B, the power, the Tonelli-Shanks steps); dense run = %.2f G products/s, "
                 "%.0f%% of the product ceiling" % (prods, prods * n / dense_ms / 1e6, 100 * prods * n / dense_ms / 1e6 / ceil[1]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    head = open(args.out).read().split(MARKER)[0] if os.path.exists(args.out) else ""  # the resource report above the marker stays
    with open(args.out, "w") as fh:
        fh.write(head + MARKER + "\n" + text + "\n")


if __name__ == "__main__":
    main()
