"""CPU-only: the arithmetic of the division kernels (polydiv.hip) replayed on the host.  fp.cuh / fz.cuh / polydiv_step.cuh are plain
C++ outside hipcc, so tests/poly_division_host_replay.cpp walks whole segments with the lane step (lazy and reduced form), builds the
transition tables by squaring the companion matrix, runs the two-level scan and the second pass from the scanned states - for
k in {1, 3, 8, 32}, lengths from k + 1 to past the second scan level, monic and non-monic divisors, on the five 4-limb fields with
edge words (0, 1, p - 1) - and compares quotient and remainder with plain fe_mul / fe_sub long division."""
from tests import hostprog


def test_division_arithmetic_replayed_on_the_host(tmp_path):
    out = hostprog.run(hostprog.build("tests/poly_division_host_replay.cpp", tmp_path, hostprog.PLAIN, extra=("-Wall",)))
    assert "mismatches: 0" in out, out
