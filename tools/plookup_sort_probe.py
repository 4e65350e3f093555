"""Timing of the Plookup sorted multiset (plookup_sort.hip) beside the grand product of the same rows, in one process.

    python tools/plookup_sort_probe.py [--field 1] [--out profiles/r11_plookup_sort.txt]

For N = 2^16, 2^18, 2^20 and two inputs - (a) t distinct, f drawn from t; (b) the padded shape of pad_inputs: half of f and a quarter
of t zero - plk_plookup_sorted_multiset_dev and plk_plookup_grand_product_dev (on the s the sort wrote), each warmed, then timed with
HIP events over REPEATS windows of CALLS back-to-back calls; median and spread per call.  Every s is compared with the counts of the
drawn indices before it is timed.  Bytes are by count, 288 N: t for the table (32 N), f and t (64 N) and each row's representative (64 N) for the counts, t_i (64 N) and s (64 N)
for the expansion; the words of the table, the counts and the offsets come on top.
"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from plonky_amd import device as dev, synth  # noqa: E402

REPEATS, CALLS = 9, 8
MARKER = "---- measured (tools/plookup_sort_probe.py) ----"


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


def inputs(fid, n, padded, seed):
    """(f_padded, t, expected s): t distinct field elements, f drawn from t; padded: the last quarter of t and the last half of f zero"""
    rng = np.random.default_rng(seed)
    t = synth.rand_field(fid, seed, n)
    assert len({r.tobytes() for r in t}) == n and t.any(axis=1).all()
    live = n - n // 4 if padded else n
    if padded:
        t[live:] = 0
    idx = rng.integers(0, live, size=n - 1)
    if padded:
        idx[(n - 1) // 2:] = live  # the first zero row of t
    f = np.concatenate([t[idx], np.zeros((1, 4), dtype=np.uint64)])
    cnt = np.bincount(idx, minlength=n)
    cnt[:live] += 1
    if padded:
        cnt[live] += n - live
    return f, t, np.repeat(t, cnt, axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "r11_plookup_sort.txt"))
    args = ap.parse_args()
    dev.init(0)
    fid = args.field
    lines = ["plookup_sort_probe: field %d, %s, %d windows of %d calls, ms per call: median (min .. max)" % (fid, torch.cuda.get_device_name(0), REPEATS, CALLS)]
    sc = synth.rand_field(fid, 5, 2)
    for log_n in (16, 18, 20):
        n = 1 << log_n
        lines.append("N = 2^%d" % log_n)
        sort_ms = {}
        for name, padded in (("a", False), ("b", True)):
            f, t, exp = inputs(fid, n, padded, 100 + log_n)
            fd, td = dev.to_device(f), dev.to_device(t)
            s, st = dev.plookup_sorted_multiset_dev(fid, log_n, fd, td, status=True)
            assert st.cpu().tolist() == [0, n - n // 4 + 1 if padded else n], st
            assert np.array_equal(dev.to_host(s), exp), "s differs from the counts"
            out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
            srt = timed(lambda: dev.plookup_sorted_multiset_dev(fid, log_n, fd, td, out=s))
            gp = timed(lambda: dev.plookup_grand_polynomial_dev(fid, log_n, fd, td, s, sc[0], sc[1], out=out))
            sort_ms[name] = srt[0]
            lines.append("  (%s) %-22s sort %8.4f (%.4f .. %.4f)  %6.1f Mrow/s  %6.1f GB/s by count (288 N bytes)   grand product %8.4f (%.4f .. %.4f)   sort / grand product = %.3f"
                         % (name, "padded: f 1/2, t 1/4 zero" if padded else "t distinct, f from t", *srt, n / srt[0] / 1e3, 288 * n / srt[0] / 1e6, *gp, srt[0] / gp[0]))
            del fd, td, s, out
            torch.cuda.empty_cache()
        lines.append("  (b) / (a) = %.3f" % (sort_ms["b"] / sort_ms["a"]))
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
