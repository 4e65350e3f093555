"""Timing probe for the gate-trace entries (run on the GPU box): 2^12 instances of the in-circuit Rescue permutation at 16 rounds and
of curve_msm at parts = 2, n_bits = 254, back to back in a device-resident table, against the same blocks generated on one host
core by the replay program (tests/gate_trace_host_replay.cpp in its `time` mode: the C++ twin of the restatement, over
gate_trace_step.cuh).  The comparison is with the host path, not with the kernel itself; it is reported, not asserted.

  python tools/gate_trace_probe.py [log_count] [host_count]
host_count instances go through the host program (default 2^7: its time is linear in the count and scaled to 2^log_count)."""
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, ".")
from oracle import bigint_ref as br  # noqa: E402
from plonky_amd import api, device as dv, synth  # noqa: E402
from tests import gate_trace_cases as gc, hostprog, rescue_ref as rr  # noqa: E402

FIELD, CURVE, ROUNDS, PARTS, N_BITS = 0, 0, 16, 2, 254


def timed(fn, reps=5, warm=1):
    """HIP events around the whole call: (median, min, max) ms"""
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def hexm(limbs):
    return "%064x" % br.limbs_to_int([int(x) for x in limbs])


def main():
    log_count = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    host_count = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 7
    count = 1 << log_count
    dv.init()
    f = br.FIELDS[FIELD]
    consts = rr.constants(FIELD, 4, ROUNDS)
    consts_limbs = np.array(rr.constants_limbs(FIELD, consts), dtype=np.uint64)
    ctx = api.RescueContext(FIELD, consts_limbs)
    inputs = synth.rand_field(FIELD, 0x7ACE, 4 * count).reshape(count, 4, 4)
    scalars = synth.rand_field(FIELD, 0x5CA1, PARTS * count).reshape(count, PARTS, 4)
    pts = np.array([[f.mont_limbs(x), f.mont_limbs(y)] for x, y in gc.points(CURVE, 1, PARTS * host_count)], dtype=np.uint64)
    points = np.resize(pts.reshape(host_count, PARTS, 2, 4), (count, PARTS, 2, 4))
    start = np.array([f.mont_limbs(v) for v in gc.start_point(CURVE)], dtype=np.uint64)
    print("gate-trace probe: %d instances, %s" % (count, torch.cuda.get_device_name(0)))
    for name, block in (("rescue", 2 * ROUNDS + 1), ("curve_msm", N_BITS * (PARTS + 1))):
        n_rows = count * block
        first = torch.arange(count, dtype=torch.int32, device="cuda") * block
        wires = torch.zeros((9, n_rows, 4), dtype=torch.int64, device="cuda")
        consts_t = torch.zeros((6, n_rows, 4), dtype=torch.int64, device="cuda")
        status = torch.zeros(4, dtype=torch.int32, device="cuda")
        if name == "rescue":
            d_in = dv.to_device(inputs)
            call = lambda k: dv.trace_rescue_permutation_dev(ctx, d_in, n_rows, first, wires=wires, constants=k, status=status)
        else:
            d_p, d_s = dv.to_device(points), dv.to_device(scalars)
            call = lambda k: dv.trace_curve_msm_dev(CURVE, d_p, d_s, start, N_BITS, n_rows, first, wires=wires, constants=k, status=status)
        for label, k in (("wires only", None), ("wires + constants", consts_t)):
            med, lo, hi = timed(lambda: call(k))
            print("%-10s %-18s rows %9d   median %10.3f ms   min %10.3f   max %10.3f   status %s"
                  % (name, label, n_rows, med, lo, hi, status.cpu().numpy().view(np.uint32).tolist()))
    # the host path: the same blocks on one core
    with tempfile.TemporaryDirectory() as tmp:
        exe = hostprog.build("tests/gate_trace_host_replay.cpp", tmp, hostprog.PLAIN)
        words = " ".join(hexm(l) for l in consts_limbs.reshape(-1, 4))
        r_block, m_block = 2 * ROUNDS + 1, N_BITS * (PARTS + 1)
        with open(tmp + "/cases.txt", "w") as fh:
            fh.write("R %d %d %s %d %d " % (FIELD, ROUNDS, words, host_count * r_block, host_count))
            fh.write(" ".join("%d %s" % (c * r_block, " ".join(hexm(x) for x in inputs[c])) for c in range(host_count)) + "\n")
            fh.write("M %d %d %d %d %d %s %s " % (FIELD, PARTS, N_BITS, host_count * m_block, host_count, hexm(start[0]), hexm(start[1])))
            fh.write(" ".join("%d %s %s" % (c * m_block, " ".join(hexm(x) for x in points[c].reshape(-1, 4)), " ".join(hexm(x) for x in scalars[c]))
                              for c in range(host_count)) + "\n")
        out = subprocess.run([exe, tmp + "/cases.txt", "time"], capture_output=True, text=True, check=True).stdout
        for line in out.strip().split("\n"):
            _, kind, n, ms = line.split()
            print("host, one core: %-9s %d instances %.1f ms -> %.1f ms for %d" % ({"R": "rescue", "M": "curve_msm"}[kind], int(n), float(ms),
                                                                               float(ms) * count / int(n), count))


if __name__ == "__main__":
    main()
