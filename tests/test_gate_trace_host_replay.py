"""CPU-only: plonky_amd/csrc/gate_trace_step.cuh (the table addressing and the block bounds, the gate prefixes, the Rescue round emitting
its rows, the add / double rows and the chain of a curve_msm instance - the code the kernels of gate_trace.hip run) compiled for the
host by tests/gate_trace_host_replay.cpp over tests/replay_io.h and compared with tests/gate_trace_ref.py: every wire and constant
written, nothing else written, the status words.  The program is built a second time under AddressSanitizer + UBSan and run on its
own (a stand-alone program: nothing of it is loaded into Python); its tables are exactly as large as n_rows says, so a block that
would pass the end must write nothing."""
import pytest

from oracle import bigint_ref as br
from tests import gate_trace_cases as gc
from tests import gate_trace_ref as gt
from tests import hostprog
from tests import rescue_ref as rr

SRC = "tests/gate_trace_host_replay.cpp"


def hexm(f, x):
    return "%064x" % f.to_mont(x % f.p)


def build_cases():
    """(kind, field, text of the case, expected (wires, constants, status))"""
    cases = []
    for field in gc.RESCUE_FIELDS:
        f = br.FIELDS[field]
        for rounds, count in ((1, 3), (2, 5)):
            consts = rr.constants(field, 4, rounds)
            block = gt.rescue_block_rows(rounds)
            v = gc.values(f, 0x900 + field + rounds, 4 * count)
            inputs = [v[4 * c:4 * c + 4] for c in range(count)]
            inputs[1] = [0, 0, 0, 0]
            n_rows = count * block + 3
            first = gc.back_to_back(count - 2, block, 1) + [n_rows - block, n_rows - block + 1]  # the last but one ends on the last row, the last passes it
            words = [hexm(f, x) for a, b in consts for x in a + b]
            text = "R %d %d %s %d %d " % (field, rounds, " ".join(words), n_rows, count)
            text += " ".join("%d %s" % (r, " ".join(hexm(f, x) for x in s)) for r, s in zip(first, inputs))
            cases.append(("R", field, text, gt.trace_rescue(field, inputs, consts, n_rows, first)))
    for curve in gc.MSM_CURVES:
        c = br.CURVES[curve]
        f, start = c.base, gc.start_point(curve)
        for parts, n_bits in ((1, 1), (2, 3), (3, 8), (8, 2), (2, f.bits - 1)):
            count = 4 if n_bits < 100 else 2
            block = gt.msm_block_rows(parts, n_bits)
            pts = gc.points(curve, parts + n_bits, count * parts)
            rnd = [x % (1 << n_bits) for x in gc.values(f, 0x3300 + curve + parts, count * parts)]
            P = [pts[i * parts:(i + 1) * parts] for i in range(count)]
            S = [rnd[i * parts:(i + 1) * parts] for i in range(count)]
            S[0] = ([0, 1, (1 << n_bits) - 1] * 3)[:parts]
            if count == 4:
                P[2] = [start] + P[2][1:]                     # the first add row meets the starting point itself
                S[1] = S[1][:-1] + [S[1][-1] | 1 << n_bits]   # a bit above n_bits
            n_rows = count * block + 2
            first = gc.back_to_back(count - 1, block, 2) + [n_rows - block + (1 if count == 4 else 0)]
            text = "M %d %d %d %d %d %s %s " % (f.field_id, parts, n_bits, n_rows, count, hexm(f, start[0]), hexm(f, start[1]))
            text += " ".join("%d %s %s" % (r, " ".join(hexm(f, x) + " " + hexm(f, y) for x, y in p), " ".join(hexm(f, s) for s in sc))
                             for r, p, sc in zip(first, P, S))
            cases.append(("M", curve, text, gt.trace_curve_msm(curve, P, S, start, n_bits, n_rows, first)))
    return cases


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gate_trace")
    cases = build_cases()
    inp = str(tmp / "cases.txt")
    with open(inp, "w") as fh:
        fh.write("\n".join(text for _, _, text, _ in cases) + "\n")
    plain = hostprog.run(hostprog.build(SRC, tmp, hostprog.PLAIN, extra=("-Wall",)), inp)
    return cases, plain, inp, tmp


def test_replay_writes_what_the_restatement_writes(replayed):
    cases, plain = replayed[:2]
    blocks, lines = [], []
    for line in plain.strip().split("\n"):  # a case ends on its status line
        lines.append(line)
        if line.startswith("S "):
            blocks.append(lines)
            lines = []
    assert len(blocks) == len(cases) and not lines
    seen_overrun = seen_exceptional = 0
    for (kind, ident, _, (wires, constants, status)), lines in zip(cases, blocks):
        f = br.FIELDS[ident] if kind == "R" else br.CURVES[ident].base
        got_status = [int(x) for x in lines[-1].split()[1:]]
        got = {"W": {}, "K": {}}
        for line in lines[:-1]:
            tag, j, row, v = line.split()
            assert (int(j), int(row)) not in got[tag]
            got[tag][(int(j), int(row))] = v
        assert got_status == status, (kind, ident)
        assert got["W"] == {k: hexm(f, v) for k, v in wires.items()}, (kind, ident)
        assert got["K"] == {k: hexm(f, v) for k, v in constants.items()}, (kind, ident)
        seen_overrun += status[0]
        seen_exceptional += status[1]
    assert seen_overrun >= len(gc.RESCUE_FIELDS) * 2 + len(gc.MSM_CURVES) * 4 and seen_exceptional >= len(gc.MSM_CURVES) * 4 * 2


def test_replay_under_the_sanitizers(replayed):
    _, plain, inp, tmp = replayed
    sanitized = hostprog.run(hostprog.build(SRC, tmp, hostprog.ASAN_UBSAN, extra=("-Wall",)), inp)
    assert sanitized == plain
