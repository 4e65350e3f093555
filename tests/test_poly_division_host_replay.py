"""CPU-only: the arithmetic of the division kernels (polydiv.hip) replayed on the host.  fp.cuh / fz.cuh / polydiv_step.cuh are plain
C++ outside hipcc, so tests/poly_division_host_replay.cpp walks whole segments with the lane step (lazy and reduced form), builds the
transition tables by squaring the companion matrix, runs the two-level scan and the second pass from the scanned states - for
k in {1, 3, 8, 32}, lengths from k + 1 to past the second scan level, monic and non-monic divisors, on the five 4-limb fields with
edge words (0, 1, p - 1) - and compares quotient and remainder with plain fe_mul / fe_sub long division."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_division_arithmetic_replayed_on_the_host(tmp_path):
    exe = str(tmp_path / "poly_division_host_replay")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "poly_division_host_replay.cpp"), "-o", exe], cwd=os.path.join(ROOT, "tests"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches: 0" in out.stdout, out.stdout + out.stderr
