"""CPU-only: the caller-buffer registry of the host-pointer entry points (plonky_amd/csrc/pin_registry.h - the code capi.hip wraps
around hipHostRegister) against a model of the runtime, in tests/pin_registry_host.cpp: a stand-alone program, built plain, with
AddressSanitizer + UBSan, and with ThreadSanitizer.  Each scenario prints the branch the registry reports for every call it makes;
the lines are compared here, so a request that silently takes another route fails although its result may be the same."""
import pytest

from tests import hostprog

# scenario -> the branches of its calls, in order (pin_registry.h: pin_branch_name; "+waited": the request slept for another thread's
# hold, "+recheckedN": the union path found the map changed under its synchronisation N times and looked again)
EXPECTED = {
    "fresh": "fresh released-last",
    "same-thread": "fresh shared released-kept released-last",
    "other-thread": "fresh shared released-kept released-last",
    "nested": "fresh shared released-kept released-last",
    "adjacent": "fresh fresh released-last released-last",
    # [0,100), [50,150), [140,300) by one thread, released with the original addresses in all six orders
    "own-union": "fresh union union released-kept released-kept released-last (6 orders)",
    # during the union's synchronisation another thread takes a hold inside the old interval / registers a range of its own in the
    # gap the union bridges / past the end the union extends: look again, wait for it, then the union
    "union-recheck": "union+waited+rechecked1 other:shared released-kept",
    "union-recheck-gap": "union+waited+rechecked1 other:fresh released-last",
    "union-recheck-beyond": "union+waited+rechecked1 other:fresh released-last",
    # hold, refused union, release of the lost hold (a no-op), the same range again, its release
    "union-fails": "fresh union-failed release-unknown fresh released-last",
    "register-fails": "register-failed fresh released-last",
    "wait-release": "union+waited other:released-kept",
    "wait-gives-up": "gave-up+waited",
    "release-not-held": "release-not-held released-last",
    "release-unknown": "release-unknown release-unknown release-unknown",
    "bridge-gap": "union released-kept released-kept released-last",
    "stress": "balanced",
}

BUILDS = {"plain": hostprog.PLAIN, "asan_ubsan": hostprog.ASAN_UBSAN, "tsan": hostprog.TSAN}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_registry_scenarios(build, tmp_path):
    out = hostprog.run(hostprog.build("tests/pin_registry_host.cpp", tmp_path, BUILDS[build], extra=hostprog.THREADS_STRICT), timeout=300)
    got = {}
    for line in out.splitlines():
        if line.startswith("scenario "):
            name, what = line[len("scenario "):].split(": ", 1)
            assert name not in got, line
            got[name] = what
    assert got == EXPECTED
    assert out.splitlines()[-1] == "OK"
