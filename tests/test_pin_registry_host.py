"""CPU-only: the caller-buffer registry of the host-pointer entry points (plonky_amd/csrc/pin_registry.h - the code capi.hip wraps
around hipHostRegister) against a model of the runtime, in tests/pin_registry_host.cpp: a stand-alone program, built plain, with
AddressSanitizer + UBSan, and with ThreadSanitizer.  Each scenario prints the branch the registry reports for every call it makes;
the lines are compared here, so a request that silently takes another route fails although its result may be the same."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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

BUILDS = {
    "plain": ["-O2"],
    "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
    "tsan": ["-O1", "-g", "-fsanitize=thread"],
}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_registry_scenarios(build, tmp_path):
    exe = str(tmp_path / ("pin_registry_host_" + build))
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "plonky_amd", "csrc"), os.path.join(ROOT, "tests", "pin_registry_host.cpp"), "-o", exe])
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
