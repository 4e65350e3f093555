"""A small set of GPU work in a child process, by default against the checked build (-DPLK_CHECKED: bounds guards that count their
violations).  One HIP library per process and knobs read once at load: hence a fresh child, selected through the environment."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKED = os.path.join(ROOT, "plonky_amd", "csrc", "libplonky_hip_checked.so")
NO_VIOLATIONS = "CHECKED violations [0, 0, 0, 0, 0, 0, 0, 0]"

PROLOGUE = '''
import os
from plonky_amd import lib
if os.environ.get("PLK_HIP_LIB") == %r:
    assert lib.load().plk_checked_build() == 1, "not the checked build"
''' % CHECKED
EPILOGUE = '''
import ctypes
from plonky_amd import lib
counts = (ctypes.c_uint * 8)()
lib.check(lib.load().plk_checked_failures(counts))
print("CHECKED violations", list(counts))
assert not any(counts), list(counts)
'''


def require_checked():
    assert os.path.exists(CHECKED), "libplonky_hip_checked.so is missing: python -c 'import __graft_entry__ as g; g.build()'"


def run_child(body, timeout=600, **env):
    """Run body between the prologue and the epilogue in a fresh Python process; returns its stdout.  The guard counters are read
    whichever library ran (the normal build reports zeros), and the line that says so must be there: a body cannot leave early."""
    out = subprocess.run([sys.executable, "-c", PROLOGUE + body + EPILOGUE], capture_output=True, text=True, timeout=timeout,
                         env=dict(os.environ, PYTHONPATH=ROOT, **env), cwd=ROOT)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert NO_VIOLATIONS in out.stdout, out.stdout[-3000:]
    return out.stdout


def run_checked(body, timeout=600):
    require_checked()
    return run_child(body, timeout, PLK_HIP_LIB=CHECKED)
