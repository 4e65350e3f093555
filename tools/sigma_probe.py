"""Timing of the copy-constraint permutation on the device (sigma.hip: plk_plonk_sigma_dev) for three partition profiles.

    python tools/sigma_probe.py [log_n] [--field 1] [--out profiles/sigma.txt]

For n = 2^16 .. 2^log_n (default 20) and three profiles of the 6n routed wires - (a) all singletons, (b) pairs, (c) one partition of
n / 2 members scattered over the columns among singletons - sigma_dev with both outputs, warmed, then timed with HIP events over REPEATS
windows of CALLS back-to-back calls; median and spread per call.  Every result is compared with the numpy neighbour rule before it is
timed.  Bytes by count per call: members read twice and offsets once (4 (2 M + P)), sigma and s_sigma written (6 n (4 + 32)); the
tables of the powers of g (32 (128 + n / 128) bytes) stay in cache.  The write bandwidth beside it is measured in this process: a fill
of a buffer of the size of s_sigma, timed the same way.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plonky_amd import device as dev, synth  # noqa: E402
from tests import sigma_cases as sc  # noqa: E402

REPEATS, CALLS = 9, 8


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


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_n", type=int, nargs="?", default=20)
    ap.add_argument("--field", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "sigma.txt"))
    args = ap.parse_args()
    dev.init(0)
    fid = args.field
    km = synth.rand_field(fid, 7, 6)
    pr = torch.cuda.get_device_properties(0)
    gpu = "%s (%s, %d CUs, %.0f GiB, uuid %s)" % (pr.name, getattr(pr, "gcnArchName", "?"), pr.multi_processor_count, pr.total_memory / 2 ** 30, getattr(pr, "uuid", "?"))
    lines = ["sigma_probe: field %d, %s, %d windows of %d calls, ms per call: median (min .. max)" % (fid, gpu, REPEATS, CALLS)]
    for log_n in range(16, args.log_n + 1):
        n = 1 << log_n
        buf = torch.empty((6 * n, 4), dtype=torch.int64, device="cuda")
        fill = timed(lambda: buf.fill_(1))
        write_bw = 6 * n * 32 / fill[0] / 1e6
        lines.append("n = 2^%d: fill of %d MiB %.4f ms (%.4f .. %.4f) = %.0f GB/s written" % (log_n, 6 * n * 32 >> 20, *fill, write_bw))
        del buf
        profiles = (("a", "all singletons", sc.singletons(n, False)), ("b", "pairs", sc.csr(sc.pair_partitions(n, 0xBEEF + log_n))),
                    ("c", "one partition of n/2", sc.skew(n, 0x5CE + log_n)))
        ms = {}
        for tag, name, (members, offsets) in profiles:
            dm, do = dev32(members), dev32(offsets)
            sigma, vals, st = dev.sigma_dev(fid, log_n, dm, do, km, status=True)
            assert st.cpu().tolist() == [0, 0, 0], st
            assert np.array_equal(sigma.cpu().numpy().view(np.uint32), sc.neighbour_rule(members, offsets, n)), "sigma differs from the neighbour rule"
            t = timed(lambda: dev.sigma_dev(fid, log_n, dm, do, km))
            ts = timed(lambda: dev.sigma_dev(fid, log_n, dm, do, km, status=True))
            moved = 4 * (2 * members.shape[0] + offsets.shape[0]) + 6 * n * 36
            written = 6 * n * 36
            ms[tag] = t[0]
            lines.append("  (%s) %-22s %8.4f (%.4f .. %.4f)  %6.1f Mwire/s  %6.1f MB moved, %6.0f GB/s; written %6.0f GB/s = %.2f of the fill   with status %8.4f (%.4f .. %.4f)"
                         % (tag, name, *t, 6 * n / t[0] / 1e3, moved / 1e6, moved / t[0] / 1e6, written / t[0] / 1e6, written / t[0] / 1e6 / write_bw, *ts))
            del dm, do, sigma, vals
            torch.cuda.empty_cache()
        lines.append("  (b) / (a) = %.3f   (c) / (a) = %.3f" % (ms["b"] / ms["a"], ms["c"] / ms["a"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
