"""CPU-only: the steps of the sorted multiset (plonky_amd/csrc/plookup_sort_step.cuh: hash, row comparison, probe step, insert, lookup,
bisection) replayed on the host by tests/plookup_sort_host_replay.cpp in the shape of the kernels, lanes in ascending and in descending
order.  The program compares every case with a first-occurrence restatement of its own; here its s is compared with
api.plookup_sorted_multiset, with tests/plookup_ref.sort_by at <= 64 rows and with the counting restatement, and the longest probe
sequence of the structured tables is bounded: host and device run the same header, so this pins the hash.  The program is built a
second time under AddressSanitizer + UBSan and run on its own (a stand-alone program: nothing of it is loaded into Python)."""
import numpy as np
import pytest

from plonky_amd import api
from tests import hostprog
from tests import plookup_ref as pr
from tests import plookup_sort_cases as sc

SRC = "tests/plookup_sort_host_replay.cpp"
SIZES = (1, 2, 6, 10)  # N = 2, 4, 64, 1024
PROBE_BOUND = 64       # at N = 1024: 2048 slots at load 1/2; a hash that clusters the structured rows runs into the hundreds


def build_cases():
    rng = np.random.default_rng(0x50F7)
    cases = []
    for log_size in SIZES:
        size = 1 << log_size
        cases.append(("distinct", log_size) + sc.distinct_case(rng, log_size))
        for first in sorted({0, 1, size - 2}):
            if first + 1 < size:
                cases.append(("duplicate of row %d" % first, log_size) + sc.duplicate_case(rng, log_size, first, size - 1))
        if size >= 4:
            cases.append(("duplicate next to row 0", log_size) + sc.duplicate_case(rng, log_size, 0, 1))
        cases.append(("padded", log_size) + sc.padded_case(rng, log_size, size // 2 - (size > 2), max(1, 3 * size // 4)))
        cases.append(("lowest word", log_size) + sc.structured_case(rng, log_size, 0))
        cases.append(("highest limb", log_size) + sc.structured_case(rng, log_size, 3))
        cases.append(("highest word", log_size) + sc.structured_case(rng, log_size, 3, 32))
        f, t = sc.distinct_case(rng, log_size)
        f[0] = 0  # distinct_rows holds no zero row: one row of f is outside t
        cases.append(("one row missing", log_size, f, t))
    return cases


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    """(cases, results of the plain build): the input file is shared with the sanitizer build"""
    tmp = tmp_path_factory.mktemp("plookup_sort")
    cases = build_cases()
    inp = str(tmp / "cases.bin")
    with open(inp, "wb") as fh:
        fh.write(np.uint32(len(cases)).tobytes())
        for _, log_size, f, t in cases:
            fh.write(np.uint32(log_size).tobytes() + f.tobytes() + t.tobytes())
    plain = hostprog.run(hostprog.build(SRC, tmp, hostprog.PLAIN, extra=("-Wall",)), inp, tmp / "out.bin")
    assert "mismatches: 0" in plain, plain
    raw, results, pos = open(str(tmp / "out.bin"), "rb").read(), [], 0
    for _, log_size, _, _ in cases:
        rows = (2 << log_size) - 1
        head = np.frombuffer(raw, dtype=np.uint32, count=3, offset=pos)
        results.append((head.tolist(), np.frombuffer(raw, dtype=np.uint64, count=rows * 4, offset=pos + 12).reshape(rows, 4)))
        pos += 12 + rows * 32
    assert pos == len(raw)
    return cases, results, plain, inp, tmp


def test_replay_matches_the_host_helper_and_the_reference_sort(replayed):
    cases, results = replayed[:2]
    for (name, log_size, f, t), ((missing, distinct, longest), s) in zip(cases, results):
        exp, exp_missing, exp_distinct = sc.restatement(f, t)
        assert (missing, distinct) == (exp_missing, exp_distinct), (name, log_size)
        assert np.array_equal(s, exp), (name, log_size)
        if missing:
            assert name == "one row missing" and missing == 1 and not s[-1].any()
            with pytest.raises(AssertionError):
                api.plookup_sorted_multiset(f[:-1], t)
            continue
        assert np.array_equal(s, api.plookup_sorted_multiset(f[:-1], t)), (name, log_size)
        if t.shape[0] <= 64:
            rows = lambda a: [tuple(int(v) for v in r) for r in a]
            assert rows(s) == pr.sort_by(rows(f[:-1]) + rows(t), rows(t)), (name, log_size)


def test_probe_sequences_stay_short(replayed):
    cases, results = replayed[:2]
    seen = 0
    for (name, log_size, _, _), ((_, _, longest), _) in zip(cases, results):
        print("%-24s N = %4d  longest probe sequence %d" % (name, 1 << log_size, longest))
        if log_size == 10:
            seen += 1
            assert longest < PROBE_BOUND, (name, longest)
        assert longest <= 2 << log_size
    assert seen >= 8


def test_replay_under_the_sanitizers(replayed):
    _, _, plain, inp, tmp = replayed
    sanitized = hostprog.run(hostprog.build(SRC, tmp, hostprog.ASAN_UBSAN, extra=("-Wall",)), inp, tmp / "out_san.bin")
    assert sanitized == plain
    assert open(str(tmp / "out_san.bin"), "rb").read() == open(str(tmp / "out.bin"), "rb").read()
