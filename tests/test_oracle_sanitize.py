"""CPU-only: the test infrastructure itself under AddressSanitizer + UndefinedBehaviorSanitizer (SURVEY.md section 5 - the
reference's own `cargo test` runs with debug assertions and overflow checks):
  * the oracle (oracle/plk_oracle.cpp + .inc files), driven by oracle/sanitize_main.cpp over every family of entry points the
    parity tests lean on;
  * the device arithmetic headers (plonky_amd/csrc/{fp,fp29,fz,ecz,glv}.cuh - exactly what the kernels compile), driven by
    tests/fp_host_sanitize_main.cpp on the host.
A finding aborts the driver (-fno-sanitize-recover); the test asserts a clean exit and the driver's own self-checks."""
import os

from tests import hostprog


def _build_and_run(tmp_path, src, marker):
    exe = hostprog.build(src, tmp_path, hostprog.ASAN_UBSAN, extra=("-pthread", "-Wall", "-Wno-unused-function"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    assert marker in hostprog.run(exe, timeout=900, env=env)


def test_oracle_under_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, "oracle/sanitize_main.cpp", "sanitize_main: ok")


def test_device_arithmetic_headers_under_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, "tests/fp_host_sanitize_main.cpp", "fp_host_sanitize: ok")
