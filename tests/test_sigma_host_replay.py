"""CPU-only: the steps of the copy-constraint permutation (plonky_amd/csrc/sigma_step.cuh: bisection, neighbour rule, id split, slot
classes, status word [0]) replayed on the host by tests/sigma_host_replay.cpp in the shape of the kernel, slots in ascending and in
descending order.  Its sigma is compared with tests/partition_ref (the reference's to_sigma, restated) up to n = 2^10 and with the numpy
neighbour rule at every size, its status words with their definitions, counted.  The program is built a second time
under AddressSanitizer + UBSan and run on its own (a stand-alone program: nothing of it is loaded into Python); both outputs must be
byte-equal."""
import numpy as np
import pytest

from tests import hostprog
from tests import partition_ref as pref
from tests import sigma_cases as sc

SRC = "tests/sigma_host_replay.cpp"


def build_cases():
    """(name, log_n, members, offsets, expected status words or None for a valid input)"""
    cases = []
    for log_n in (0, 1, 2):
        cases.append(("singletons",) + (log_n,) + sc.singletons(1 << log_n) + (None,))
        cases.append(("routed singletons only",) + (log_n,) + sc.singletons(1 << log_n, False) + (None,))
    for log_n in (2, 8):
        cases.append(("one cycle", log_n) + sc.one_cycle(1 << log_n, 0xC1C + log_n) + (None,))
    for name, (m, o) in sc.listing_variants(16, 0x715).items():
        cases.append((name, 4, m, o, None))
    cases.append(("seams", 10) + sc.seams(1 << 10, 0x5EA) + (None,))
    for log_n, cap in ((2, None), (4, None), (10, None), (16, 32)):
        n = 1 << log_n
        ops = sc.merge_sequence(n, 0xAB0 + log_n, n_virtual=max(2, n // 4), n_merges=3 * n, cap=cap)
        tp = sc.build_partitions(pref.TargetPartitionsRef, n, ops, max(2, n // 4))
        wp = tp.to_wire_partitions()
        live = sorted(set(wp.indices.values()))
        cases.append(("random merges", log_n) + sc.csr([[i * n + g for g, i in wp.partitions[q]] for q in live]) + (None,))
    for name, (m, o, st) in sc.bad_cases(16, 0x715).items():
        cases.append((name, 4, m, o, st))
    cases.append(("id = 9n", 4) + sc.out_of_range_case(16, 1))
    return cases


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sigma")
    cases = build_cases()
    inp = str(tmp / "cases.bin")
    with open(inp, "wb") as fh:
        fh.write(np.uint32(len(cases)).tobytes())
        for _, log_n, m, o, _ in cases:
            fh.write(np.array([log_n, o.shape[0] - 1, m.shape[0]], dtype=np.uint32).tobytes() + o.tobytes() + m.tobytes())
    plain = hostprog.run(hostprog.build(SRC, tmp, hostprog.PLAIN, extra=("-Wall",)), inp, tmp / "out.bin")
    assert "mismatches: 0" in plain, plain
    raw, results, pos = open(str(tmp / "out.bin"), "rb").read(), [], 0
    for _, log_n, _, _, _ in cases:
        n6 = 6 << log_n
        words = np.frombuffer(raw, dtype=np.uint32, count=3 + 3 * n6, offset=pos)
        results.append((words[:3].tolist(), words[3:3 + n6], words[3 + n6:3 + 2 * n6], words[3 + 2 * n6:]))
        pos += 4 * (3 + 3 * n6)
    assert pos == len(raw)
    return cases, results, plain, inp, tmp


def test_replay_matches_the_reference_and_the_neighbour_rule(replayed):
    cases, results = replayed[:2]
    names = set()
    for (name, log_n, m, o, bad), (status, sigma, inp, gate) in zip(cases, results):
        n = 1 << log_n
        names.add(name)
        assert status == pref.status_words_ref(m, o, n) == (bad or [0, 0, 0]), (name, log_n, status)
        if bad:
            continue
        assert np.array_equal(sigma, sc.neighbour_rule(m, o, n)), (name, log_n)
        assert np.array_equal(inp.astype(np.int64) * n + gate, sigma), (name, log_n)  # the id split
        assert inp.max() < 6 and gate.max() < n
        if log_n <= 10:
            wp = pref.csr_to_wire_partitions(m, o, n)
            for g in range(n):  # the non-routed wires a listing leaves out: to_sigma only counts them (partition.rs:124-125)
                for i in range(pref.NUM_WIRES):
                    wp.indices.setdefault((g, i), -1)
            assert sigma.tolist() == wp.to_sigma(), (name, log_n)
    assert {"id = 9n", "one wire listed twice", "one wire left out", "a non-routed wire in a pair", "seams", "random merges"} <= names


def test_reference_refuses_what_the_status_words_count(replayed):
    """the restated reference panics on the defects that set a status word"""
    for name, log_n, m, o, bad in replayed[0]:
        if not bad or name == "id = 9n":
            continue
        n = 1 << log_n
        wp = pref.csr_to_wire_partitions(m, o, n)
        if bad[1]:
            with pytest.raises(AssertionError, match="Non-routed wires"):
                wp.assert_valid()
        elif name == "one wire left out":
            for g in range(n):
                for i in range(pref.NUM_WIRES):
                    if i >= pref.NUM_ROUTED_WIRES:
                        wp.indices.setdefault((g, i), -1)
            wp.indices[("pad", 0)] = -1  # keeps the count of wires a multiple of NUM_WIRES: the panic is the lookup, not the debug_assert
            with pytest.raises(KeyError):
                wp.to_sigma()


def test_replay_under_the_sanitizers(replayed):
    _, _, plain, inp, tmp = replayed
    sanitized = hostprog.run(hostprog.build(SRC, tmp, hostprog.ASAN_UBSAN, extra=("-Wall",)), inp, tmp / "out_san.bin")
    assert sanitized == plain
    assert open(str(tmp / "out_san.bin"), "rb").read() == open(str(tmp / "out.bin"), "rb").read()
