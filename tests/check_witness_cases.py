"""The refusals of plk_plonk_check_witness[_dev] (include/plonky_hip_witness.h) as data, shared by the CPU test that pins their codes and
texts (tests/test_check_witness_abi.py, tests/golden/check_witness_refusals.json) and the GPU test that sees the same ones with a device
present, and the fault planting of the satisfied circuit.  A plain helper module: no fixtures, no pytest settings."""
import ctypes

import numpy as np

ENTRIES = ("plk_plonk_check_witness_dev", "plk_plonk_check_witness")

# name -> (overrides of the good call, the text plk_last_error starts with); arguments by name, the stream of the device form aside
GOOD = dict(log_degree=2, field=0, constants="p", constants_stride=1, wires="p", sigma="p", inner_zeta="p", inner_a="p", report="p", row_masks="p",
            first_terms="p")
ORDER = ("log_degree", "field", "constants", "constants_stride", "wires", "sigma", "inner_zeta", "inner_a", "report", "row_masks", "first_terms")
REFUSALS = [
    ("unknown field -1", dict(field=-1), "bad field id -1"),
    ("unknown field 6", dict(field=6), "bad field id 6"),
    ("unknown field 1000", dict(field=1000), "bad field id 1000"),
    ("six-limb field", dict(field=3), "field 3 has 6 limbs"),
    ("log_degree 28", dict(log_degree=28), "log_degree 28"),
    ("log_degree 4000000000", dict(log_degree=4000000000), "log_degree 4000000000"),
    ("stride 0", dict(constants_stride=0), "constants_stride 0"),
    ("stride 2", dict(constants_stride=2), "constants_stride 2"),
    ("stride 4", dict(constants_stride=4), "constants_stride 4"),
    ("stride 16", dict(constants_stride=16), "constants_stride 16"),
    ("null constants", dict(constants=None), "null pointer: constants"),
    ("null wires", dict(wires=None), "null pointer: wires"),
    ("null report", dict(report=None), "null pointer: report"),
    ("null inner_zeta", dict(inner_zeta=None), "null pointer: inner_zeta"),
    ("null inner_a", dict(inner_a=None), "null pointer: inner_a"),
    # the order of the checks: the field before the size, the size before the stride, the stride before the pointers
    ("unknown field and log_degree 28", dict(field=9, log_degree=28), "bad field id 9"),
    ("log_degree 28 and stride 3", dict(log_degree=28, constants_stride=3), "log_degree 28"),
    ("stride 3 and everything null", dict(constants_stride=3, constants=None, wires=None, report=None, inner_zeta=None, inner_a=None), "constants_stride 3"),
    ("everything null", dict(constants=None, wires=None, sigma=None, report=None, row_masks=None, first_terms=None, inner_zeta=None, inner_a=None),
     "null pointer: constants"),
]


def refusal_results(L):
    """[(entry, case name, code, text)] of every refusal through both entries of the loaded library L; the pointers of the good call all
    name one small host buffer that no refused call reads"""
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    out = []
    for entry in ENTRIES:
        for name, override, _ in REFUSALS:
            args = [dict(GOOD, **override)[k] for k in ORDER]
            args = [p if a == "p" else a for a in args]
            if entry.endswith("_dev"):
                args.append(None)  # the stream
            rc = getattr(L, entry)(*args)
            out.append((entry, name, int(rc), L.plk_last_error().decode()))
    return out


def break_row(wires, row, value, period=None):
    """Spoil gate `row` of tests.test_gpu_plonk.honest_tables (gate kinds cycle with the row index mod 5, within a tile of `period`
    rows when the table is a tiling) by writing `value` (4 limbs) into one wire that only this row's own gate reads: the output of
    an ArithmeticGate, the wire of a ConstantGate, the sum of a Base4SumGate, y_new of a CurveDblGate."""
    kind = (row % period if period else row) % 5
    wires[{0: 3, 1: 0, 2: 1, 3: 0, 4: 3}[kind], row] = value
