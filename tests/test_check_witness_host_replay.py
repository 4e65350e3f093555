"""CPU-only: the steps of the witness check that hold no field arithmetic (plonky_amd/csrc/witness_step.cuh: the right / below row
indices, the class of a sigma entry, the wave-to-report merge) replayed on the host by tests/check_witness_host_replay.cpp in the shape
of the kernels, the waves in ascending and in descending order.  The report is compared with its definition in numpy, the indices
with (i + 1) % n and (i + 65) % n - n = 1 .. 64 wrap the below index more than once.  The wire buffer holds the 6n routed elements
and nothing behind them, so the build under AddressSanitizer + UBSan (a stand-alone program: nothing of it is loaded into Python)
also shows that a sigma entry >= 6n is never followed; both outputs must be byte-equal."""
import numpy as np
import pytest

from tests import hostprog

SRC = "tests/check_witness_host_replay.cpp"
NONE = 0xFFFFFFFF


def build_cases():
    """(name, log_n, masks (n,) uint8, wires (6n, 8) uint32, sigma (6n,) uint32 or None)"""
    cases = []
    for log_n in range(0, 9):
        n = 1 << log_n
        rng = np.random.default_rng(0x17E5 + log_n)
        wires = rng.integers(0, 4, (6 * n, 8), dtype=np.uint32)  # few values: equal elements happen, and elements that differ in one word
        wires[:, 1:] = 0
        wires[rng.integers(0, 6 * n, max(1, n // 2)), rng.integers(1, 8, max(1, n // 2))] = 1
        sigma = rng.permutation(6 * n).astype(np.uint32)
        cases.append(("clean", log_n, np.zeros(n, dtype=np.uint8), wires, np.arange(6 * n, dtype=np.uint32)))
        cases.append(("random", log_n, (rng.integers(0, 256, n) * (rng.random(n) < 0.3)).astype(np.uint8), wires, sigma))
        cases.append(("no sigma", log_n, rng.integers(0, 256, n).astype(np.uint8), wires, None))
        far = sigma.copy()
        far[rng.integers(0, 6 * n, 3)] = [6 * n, NONE, 9 * n - 1]
        cases.append(("sigma out of range", log_n, np.zeros(n, dtype=np.uint8), wires, far))
    n = 1 << 8
    for row in (0, 63, 64, 127, 128, n - 1):  # one failing row at the edges of a wave and of a workgroup
        m = np.zeros(n, dtype=np.uint8)
        m[row] = 1 + row % 255
        cases.append(("row %d" % row, 8, m, np.zeros((6 * n, 8), dtype=np.uint32), None))
    return cases


def expected(log_n, masks, wires, sigma):
    n = 1 << log_n
    bad = np.flatnonzero(masks)
    words = [bad.shape[0], int(bad[0]) if bad.shape[0] else NONE, int(masks[bad[0]]) if bad.shape[0] else 0, 0, NONE, 0, 0, 0]
    if sigma is not None:
        s = sigma.astype(np.int64)
        inside = s < 6 * n
        d = np.zeros(6 * n, dtype=bool)
        d[inside] = (wires[inside] != wires[s[inside]]).any(axis=1)
        w = np.flatnonzero(d)
        words[3:6] = [w.shape[0], int(w[0]) if w.shape[0] else NONE, int((~inside).sum())]
    return words


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("witness")
    cases = build_cases()
    inp = str(tmp / "cases.bin")
    with open(inp, "wb") as fh:
        fh.write(np.uint32(len(cases)).tobytes())
        for _, log_n, masks, wires, sigma in cases:
            fh.write(np.array([log_n, 0 if sigma is None else 1], dtype=np.uint32).tobytes() + masks.tobytes() + np.ascontiguousarray(wires).tobytes())
            if sigma is not None:
                fh.write(sigma.tobytes())
    plain = hostprog.run(hostprog.build(SRC, tmp, hostprog.PLAIN, extra=("-Wall",)), inp, tmp / "out.bin")
    assert "order mismatches: 0" in plain, plain
    return cases, plain, inp, tmp


def test_replay_matches_the_definitions(replayed):
    cases, _, _, tmp = replayed
    raw, pos = open(str(tmp / "out.bin"), "rb").read(), 0
    seen = set()
    for name, log_n, masks, wires, sigma in cases:
        n = 1 << log_n
        words = np.frombuffer(raw, dtype=np.uint32, count=8 + 2 * n, offset=pos)
        pos += 4 * (8 + 2 * n)
        assert words[:8].tolist() == expected(log_n, masks, wires, sigma), (name, log_n)
        i = np.arange(n)
        assert np.array_equal(words[8:8 + n], (i + 1) % n) and np.array_equal(words[8 + n:], (i + 65) % n), (name, log_n)
        if name == "sigma out of range":
            assert words[5] >= 1
        if name == "random" and log_n >= 4:
            assert words[0] > 1 and words[3] > 1
        seen.add(name)
    assert pos == len(raw) and {"clean", "random", "no sigma", "sigma out of range", "row 63", "row 64", "row 128"} <= seen


def test_replay_under_the_sanitizers(replayed):
    _, plain, inp, tmp = replayed
    sanitized = hostprog.run(hostprog.build(SRC, tmp, hostprog.ASAN_UBSAN, extra=("-Wall",)), inp, tmp / "out_san.bin")
    assert sanitized == plain
    assert open(str(tmp / "out_san.bin"), "rb").read() == open(str(tmp / "out.bin"), "rb").read()
