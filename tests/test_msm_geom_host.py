"""CPU-only: the MSM's geometry (plonky_amd/csrc/msm_geom.h: window, partition, reduction shape, chunking, workspace sizes), compiled
for the host with g++ - it is plain C++ - and swept for what the kernels assume of it.  The same header, so the same arithmetic, that
msm.hip configures every context with."""
import ctypes

import pytest

from tests import hostprog

TWEEDLEDEE, BLS12_377 = 0, 2


@pytest.fixture(scope="module")
def geom_lib(tmp_path_factory):
    L = ctypes.CDLL(hostprog.build_shared("tests/msm_geom_host.cpp", tmp_path_factory.mktemp("msm_geom")))
    L.msm_geom_check_grid.restype = ctypes.c_long
    L.msm_geom_check_grid.argtypes = [ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long), ctypes.c_char_p, ctypes.c_size_t]
    L.msm_geom_auto_window.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_int]
    return L


def test_every_geometry_is_one_the_kernels_can_run(geom_lib):
    """All five curves x n in {0, 1, 2, 3, 31, 1000, 6000, 2^k - 1, 2^k, 2^k + 1 (k = 10 .. 24), 349525, 1000003} x twelve window requests x
    tabled / table-free x three lane counts x fifteen knob settings: a geometry that is not refused satisfies the bounds of the ordering
    (bins, fine bits, tile), of the reduction (grid split, planes, parts), of the chunking, and a halving sequence fits the workspace
    sized for it (msm_geom_host.cpp lists the requirements)."""
    rows, refused = ctypes.c_long(), ctypes.c_long()
    msg = ctypes.create_string_buffer(256)
    bad = geom_lib.msm_geom_check_grid(ctypes.byref(rows), ctypes.byref(refused), msg, len(msg))
    assert bad == 0, "%d violations, the first: %s" % (bad, msg.value.decode())
    assert rows.value > 300000 and 0 < refused.value < rows.value // 2  # the sweep ran, and mostly on geometries that exist


@pytest.mark.parametrize("curve,n,table_free,window", [
    (TWEEDLEDEE, 1 << 14, 0, 16),
    (TWEEDLEDEE, 1 << 16, 0, 16),
    (TWEEDLEDEE, 1 << 18, 0, 16),
    (TWEEDLEDEE, 1 << 20, 0, 20),
    (BLS12_377, 1 << 19, 0, 17),
    (TWEEDLEDEE, 1 << 20, 1, 16),
    (BLS12_377, 1 << 20, 1, 15),
])
def test_window_of_the_tracked_sizes(geom_lib, curve, n, table_free, window):
    """The automatic window at the sizes BASELINE.md tracks: a change of choose_window shows up here before it shows up as a timing."""
    assert geom_lib.msm_geom_auto_window(curve, n, table_free) == window
