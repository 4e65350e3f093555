"""Stand-alone C++ host programs for the CPU-only tests: one place that names the compiler, the flag sets and what a clean run is.
A sanitized build is a program of its own; nothing sanitized is ever loaded into Python (build_shared takes no flavour)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky_amd", "csrc")

PLAIN = ("-O2",)
ASAN_UBSAN = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
TSAN = ("-O1", "-g", "-fsanitize=thread")
THREADS_STRICT = ("-pthread", "-Wall", "-Wextra", "-Werror")  # the table cache and the pin registry
MARKS = ("Sanitizer", "runtime error", "VIOLATION", "WARNING:")  # what no stream of a clean run holds, whatever the flavour


def _compile(src, out, flags):
    cmd = ["g++", "-std=c++17", "-I" + CSRC, *flags, os.path.join(ROOT, src), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout[-2000:] + p.stderr[-4000:]
    return out


def build(src, out_dir, flavour, extra=()):
    """Compile src (a path under the repository root) with a flavour's flags; returns the executable."""
    tag = {PLAIN: "plain", ASAN_UBSAN: "asan_ubsan", TSAN: "tsan"}[flavour]
    return _compile(src, os.path.join(str(out_dir), "%s_%s" % (os.path.splitext(os.path.basename(src))[0], tag)), flavour + tuple(extra))


def build_shared(src, out_dir):
    """Compile a ctypes harness, plain flags only; returns the .so."""
    return _compile(src, os.path.join(str(out_dir), os.path.splitext(os.path.basename(src))[0] + ".so"), PLAIN + ("-shared", "-fPIC"))


def run(exe, *args, timeout=600, env=None):
    """Run a built program to a clean end and return its stdout."""
    p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=env)
    report = "stdout: ...%s\nstderr: ...%s" % (p.stdout[-2000:], p.stderr[-4000:])
    assert p.returncode == 0, "%s: exit %d\n%s" % (os.path.basename(exe), p.returncode, report)
    for mark in MARKS:
        assert mark not in p.stdout and mark not in p.stderr, "%s: %r in its output\n%s" % (os.path.basename(exe), mark, report)
    return p.stdout
