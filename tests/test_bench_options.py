"""CPU: the command line of bench.py (a plain run unless --full) and the file format of --dump-outputs."""
import os

import numpy as np

from benchlib.common import DUMP_LIMIT_BYTES, DUMP_SAMPLE_ROWS, dump_outputs, parse_args


def test_plain_run_is_the_default():
    a = parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_exact_halves_and_fixed_sample(tmp_path):
    """uint64 limbs come back exactly from the float64 halves; an output above DUMP_SAMPLE_ROWS rows is the same sorted sample in
    every call; the total stays under the limit."""
    rng = np.random.default_rng(5)
    small = rng.integers(0, 2 ** 63, size=(100, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    big = rng.integers(0, 2 ** 63, size=(DUMP_SAMPLE_ROWS + 77, 4), dtype=np.uint64)
    flags = np.array([0, 1], dtype=np.uint8)
    shapes = dump_outputs(str(tmp_path / "a"), [("small", small), ("big", big), ("flags", flags)])
    assert shapes == {"small": [100, 8], "big": [DUMP_SAMPLE_ROWS, 8], "flags": [2]}
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s.astype(np.uint32).view(np.uint64), small)
    assert np.array_equal(np.load(tmp_path / "a" / "flags.npy"), [0.0, 1.0])
    b = np.load(tmp_path / "a" / "big.npy").astype(np.uint32).view(np.uint64)
    rows = {tuple(r) for r in big.tolist()}
    assert all(tuple(r) in rows for r in b[:1000].tolist())
    dump_outputs(str(tmp_path / "b"), [("big", big)])
    assert np.array_equal(np.load(tmp_path / "b" / "big.npy"), np.load(tmp_path / "a" / "big.npy"))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= DUMP_LIMIT_BYTES + 4096
