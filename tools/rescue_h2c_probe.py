"""Timing of the Rescue hash to the curve on the device (rescue_h2c.hip).

    python tools/rescue_h2c_probe.py [--out profiles/rescue_h2c.txt]

plk_rescue_hash_to_curve_dev on Tweedledee at 16 rounds for 2^10, 2^14 and 2^16 seeds: warmed, timed with HIP events over REPEATS
windows, median and spread per call.  Beside each, in the same process: plk_hash_to_curve_dev (the BLAKE3 form: the comparison the
reference's benches/hash_to_curve.rs makes) at the same count, and plk_rescue_sponge_dev on 2 x count rows of 2 inputs and 2 outputs
(the expected number of permutations).  The loop form (PLK_H2C_NAIVE=1, read once) is timed by a child process of the same run.  The
figures go under a marker line of the output file; the resource report above it stays.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plonky_amd import api, device as dev, synth  # noqa: E402

REPEATS = 7
ROUNDS = 16
LOGS = (10, 14, 16)
CURVE = 0  # Tweedledee
MARKER = "---- measured (tools/rescue_h2c_probe.py) ----"


def timed(fn, calls=2):
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


def fmt(ms):
    return "%9.3f (%9.3f .. %9.3f)" % ms


def rescue_times(ctx):
    res = {}
    for log_n in LOGS:
        n = 1 << log_n
        out = torch.empty((n, 2, 4), dtype=torch.int64, device="cuda")
        res[log_n] = timed(lambda: dev.rescue_hash_to_curve_dev(ctx, CURVE, n, out=out))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "rescue_h2c.txt"))
    ap.add_argument("--child", action="store_true", help="print the Rescue timings alone (the parent sets PLK_H2C_NAIVE)")
    args = ap.parse_args()
    dev.init(0)
    ctx = api.RescueContext(0, synth.rand_field(0, 1337, ROUNDS * 2 * 4).reshape(ROUNDS, 2, 4, -1))
    mine = rescue_times(ctx)
    if args.child:
        for log_n in LOGS:
            print("CHILD %d %.6f %.6f %.6f" % ((log_n,) + mine[log_n]))
        return
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, PLK_H2C_NAIVE="1"), cwd=ROOT)
    assert child.returncode == 0, (child.stdout + child.stderr)[-2000:]
    loop = {int(l.split()[1]): tuple(float(v) for v in l.split()[2:5]) for l in child.stdout.splitlines() if l.startswith("CHILD ")}
    lines = ["rescue_h2c_probe: %s, %d windows of 2 calls, warmed, HIP events, ms per call: median (min .. max); Tweedledee, %d rounds"
             % (torch.cuda.get_device_name(0), REPEATS, ROUNDS)]
    for log_n in LOGS:
        n = 1 << log_n
        out = torch.empty((n, 2, 4), dtype=torch.int64, device="cuda")
        blake = timed(lambda: dev.hash_to_curve_dev(CURVE, n, out=out))
        inp = dev.to_device(synth.rand_field(0, 9, 2 * 2 * n).reshape(2 * n, 2, -1))
        sout = torch.empty((2 * n, 2, 4), dtype=torch.int64, device="cuda")
        sponge = timed(lambda: dev.rescue_sponge_dev(ctx, inp, 2, out=sout))
        lines.append("2^%d seeds" % log_n)
        lines.append("  plk_rescue_hash_to_curve_dev, rounds over a compacted list   %s   %.3f M points/s" % (fmt(mine[log_n]), n / mine[log_n][0] / 1e3))
        lines.append("  plk_rescue_hash_to_curve_dev, loop form (PLK_H2C_NAIVE=1)    %s   loop / rounds x%.2f" % (fmt(loop[log_n]), loop[log_n][0] / mine[log_n][0]))
        lines.append("  plk_hash_to_curve_dev (BLAKE3), same count                   %s   Rescue / BLAKE3 x%.1f" % (fmt(blake), mine[log_n][0] / blake[0]))
        lines.append("  plk_rescue_sponge_dev, 2 x count rows of 2 -> 2               %s   hash / sponge x%.2f" % (fmt(sponge), mine[log_n][0] / sponge[0]))
    ctx.free()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    head = open(args.out).read().split(MARKER)[0] if os.path.exists(args.out) else ""  # the resource report above the marker stays
    with open(args.out, "w") as fh:
        fh.write(head + MARKER + "\n" + text + "\n")


if __name__ == "__main__":
    main()
