"""Timing of Rescue on the device (rescue.hip): batched permutations, the sponge and k-th roots.

    python tools/rescue_probe.py [--out profiles/rescue.txt]

plk_rescue_permutation_dev for 2^10, 2^14 and 2^18 states on TweedledeeBase and 2^14 on Bls12377Base (16 rounds), plk_rescue_sponge_dev
at 2 inputs and 2 outputs (the shape of hash_base_field_to_curve) for 2^14 rows, plk_field_kth_root_dev (k = 5) for 2^20 elements:
warmed, timed with HIP events over REPEATS windows, median and spread per call.  Beside each, the field products per second by count
(the exponent's 4-bit digits, the x^alpha chain, four products per matrix row) and the fraction of the product-chain ceiling
plk_bench_ceilings measures in this process.  The figures go under a marker line of the output file; the resource report above it stays.
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plonky_amd import api, device as dev, lib, synth  # noqa: E402

REPEATS = 9
ROUNDS = 16
MARKER = "---- measured (tools/rescue_probe.py) ----"
NAMES = {0: "TweedledeeBase", 3: "Bls12377Base"}
ALPHA = {0: 5, 3: 5}
KERNEL_WAVES = {0: 4, 3: 2}  # waves per SIMD of k_rescue_permute, from the resource report


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


def root_exponent(p, k):  # field.rs:346-375
    num = p
    for _ in range(k):
        num += p - 1
        if num % k == 0:
            return (num // k) % (p - 1)
    raise ValueError(k)


def chain_products(d):
    """products of the windowed chain x^d: the odd-power table (1 + 7), four squarings per digit below the top, one product per
    non-zero digit below the top"""
    digits = [(d >> s) & 15 for s in range(0, d.bit_length(), 4)]
    return 8 + 4 * (len(digits) - 1) + sum(1 for g in digits[:-1] if g)


def permutation_products(field):
    """per state: W elements x rounds x (the root chain, the x^alpha chain, two matrix rows of W products)"""
    a = ALPHA[field]
    return 4 * ROUNDS * (chain_products(root_exponent(synth.MODULI[field], a)) + {5: 3, 11: 5}[a] + 2 * 4)


def context(field):
    consts = synth.rand_field(field, 1337, ROUNDS * 2 * 4).reshape(ROUNDS, 2, 4, -1)
    return api.RescueContext(field, consts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "rescue.txt"))
    args = ap.parse_args()
    dev.init(0)
    lines = ["rescue_probe: %s, %d windows, ms per call: median (min .. max); %d rounds" % (torch.cuda.get_device_name(0), REPEATS, ROUNDS)]
    ceil = (ctypes.c_double * 8)()
    lib.check(lib.load().plk_bench_ceilings(ceil, 8))
    ceiling = {0: ceil[1], 3: ceil[2]}
    lines.append("plk_bench_ceilings: Montgomery product chains at 4 waves per SIMD: %.2f G/s (9 limbs), %.2f G/s (14 limbs); k_rescue_permute holds "
                 "%d and %d waves per SIMD" % (ceil[1], ceil[2], KERNEL_WAVES[0], KERNEL_WAVES[3]))

    def report(name, field, n, ms, products):
        rate = products * n / ms[0] / 1e6
        lines.append("%-44s %9.3f (%9.3f .. %9.3f)   %8.3f M/s   %7.2f G products/s   %3.0f%% of the ceiling"
                     % (name, ms[0], ms[1], ms[2], n / ms[0] / 1e3, rate, 100 * rate / ceiling[field]))

    ctxs = {f: context(f) for f in (0, 3)}
    for field, log_n in ((0, 10), (0, 14), (0, 18), (3, 14)):
        n = 1 << log_n
        states = dev.to_device(synth.rand_field(field, 7, 4 * n).reshape(n, 4, -1))
        out = torch.empty_like(states)
        ms = timed(lambda: dev.rescue_permutation_dev(ctxs[field], states, out=out), 2 if log_n >= 18 else 4)
        report("permutation %s 2^%d (%d products each)" % (NAMES[field], log_n, permutation_products(field)), field, n, ms, permutation_products(field))
    n = 1 << 14
    inp = dev.to_device(synth.rand_field(0, 9, 2 * n).reshape(n, 2, -1))
    out = torch.empty((n, 2, 4), dtype=torch.int64, device="cuda")
    ms = timed(lambda: dev.rescue_sponge_dev(ctxs[0], inp, 2, out=out), 4)
    report("sponge 2 -> 2 TweedledeeBase 2^14 (1 permutation)", 0, n, ms, permutation_products(0))
    n = 1 << 20
    x = dev.to_device(synth.rand_field(0, 11, n))
    out = torch.empty_like(x)
    per_root = chain_products(root_exponent(synth.MODULI[0], 5)) + 2  # the chain, and the two products that enter and leave the working form
    ms = timed(lambda: dev.kth_root_dev(0, x, 5, out=out), 2)
    report("kth_root k = 5 TweedledeeBase 2^20 (%d products each)" % per_root, 0, n, ms, per_root)
    for c in ctxs.values():
        c.free()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    head = open(args.out).read().split(MARKER)[0] if os.path.exists(args.out) else ""  # the resource report above the marker stays
    with open(args.out, "w") as fh:
        fh.write(head + MARKER + "\n" + text + "\n")


if __name__ == "__main__":
    main()
