"""CPU-only: the arithmetic of the opening kernels (opening.hip) replayed on the host.  fp.cuh / fz.cuh are plain C++ outside hipcc, so
tests/opening_host_replay.cpp walks the evaluation tile by tile and lane by lane (rows of six products through one reduction, the
x^l and x^(tile) factors, tails inside a row and a tile), the reduction's running total over 40 polynomials and the two-level sum of
halo_b at 8 points, on the five 4-limb fields with edge words, and compares each result with plain fe_mul / fe_add arithmetic."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_opening_arithmetic_replayed_on_the_host(tmp_path):
    exe = str(tmp_path / "opening_host_replay")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "opening_host_replay.cpp"), "-o", exe], cwd=os.path.join(ROOT, "tests"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches: 0" in out.stdout, out.stdout + out.stderr
