"""CPU-only: the cache of device-resident tables (plonky_amd/csrc/table_cache.h - the one rule behind the NTT plans, the Plonk and
Plookup circuit-size tables and the tables of poly.hip) with a counting struct in place of device buffers, in
tests/table_cache_host.cpp: a stand-alone program, built plain, with AddressSanitizer + UBSan, and with ThreadSanitizer.  Each
scenario prints one line with what it counted; the lines are compared here."""
import pytest

from tests import hostprog

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

BUILDS = {"plain": hostprog.PLAIN, "asan_ubsan": hostprog.ASAN_UBSAN, "tsan": hostprog.TSAN}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_table_cache_scenarios(build, tmp_path):
    out = hostprog.run(hostprog.build("tests/table_cache_host.cpp", tmp_path, BUILDS[build], extra=hostprog.THREADS_STRICT), timeout=300)
    got = {}
    for line in out.splitlines():
        if line.startswith("scenario "):
            name, what = line[len("scenario "):].split(": ", 1)
            assert name not in got, line
            got[name] = what
    assert got == EXPECTED
    assert out.splitlines()[-1] == "OK"
