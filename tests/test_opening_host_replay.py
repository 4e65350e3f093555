"""CPU-only: the arithmetic of the opening kernels (opening.hip) replayed on the host.  fp.cuh / fz.cuh are plain C++ outside hipcc, so
tests/opening_host_replay.cpp walks the evaluation tile by tile and lane by lane (rows of six products through one reduction, the
x^l and x^(tile) factors, tails inside a row and a tile), the reduction's running total over 40 polynomials and the two-level sum of
halo_b at 8 points, on the five 4-limb fields with edge words, and compares each result with plain fe_mul / fe_add arithmetic."""
from tests import hostprog


def test_opening_arithmetic_replayed_on_the_host(tmp_path):
    out = hostprog.run(hostprog.build("tests/opening_host_replay.cpp", tmp_path, hostprog.PLAIN, extra=("-Wall",)))
    assert "mismatches: 0" in out, out
