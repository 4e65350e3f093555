"""CPU-only: the cache of device-resident tables (plonky_amd/csrc/table_cache.h - the one rule behind the NTT plans, the Plonk and
Plookup circuit-size tables and the tables of poly.hip) with a counting struct in place of device buffers, in
tests/table_cache_host.cpp: a stand-alone program, built plain, with AddressSanitizer + UBSan, and with ThreadSanitizer.  Each
scenario prints one line with what it counted; the lines are compared here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = {
    # a second get of a key runs no build and returns the same pointer
    "hit-and-miss": "rc 0 0 0 builds 2 same 1 distinct 1 alive 2",
    # PLK_ERR_OOM (-7) comes back, `out` stays empty, the half-built object is constructed and destroyed exactly once before get
    # returns, and the next get of the key builds again
    "failed-build": "rc -7 then 0 builds 2 out-empty 1 half-built constructed 1 destroyed 1 got-key 1",
    # max_entries = 4, keys 0..5 inserted in order: the 4 largest stay; the evicted two die only when the test lets go of them
    "bound": "kept [2 3 4 5] evicted destroyed while held 0 after release 1 1",
    "clear-under-hold": "absent 1 destroyed after clear 0 held-key 3 destroyed after release 1 at end 1",
    # cache a's build takes a table of cache b; a hit in a does not ask b; table_caches_clear empties both
    "nested": "rc 0 0 0 builds a 2 b 2",
    "stress": "balanced",
}

BUILDS = {
    "plain": ["-O2"],
    "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
    "tsan": ["-O1", "-g", "-fsanitize=thread"],
}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_table_cache_scenarios(build, tmp_path):
    exe = str(tmp_path / ("table_cache_host_" + build))
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "plonky_amd", "csrc"), os.path.join(ROOT, "tests", "table_cache_host.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    report = p.stdout[-4000:] + p.stderr[-4000:]
    assert p.returncode == 0, report
    for mark in ("VIOLATION", "Sanitizer", "runtime error", "WARNING:"):
        assert mark not in p.stdout and mark not in p.stderr, report
    got = {}
    for line in p.stdout.splitlines():
        if line.startswith("scenario "):
            name, what = line[len("scenario "):].split(": ", 1)
            assert name not in got, line
            got[name] = what
    assert got == EXPECTED
    assert p.stdout.splitlines()[-1] == "OK"
