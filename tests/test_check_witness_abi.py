"""CPU-only: the witness-check entries (plk_plonk_check_witness[_dev]) are declared in a header of their own,
include/plonky_hip_witness.h, size first; lib.WITNESS_SYMBOLS binds exactly what that header declares, apart from lib.SYMBOLS (which mirrors
include/plonky_hip.h); both libraries export them; every refusal comes back with its code and its own text before a device is
selected (tests/golden/check_witness_refusals.json, recorded from this build), and a good call without a GPU is PLK_ERR_NO_DEVICE."""
import ctypes
import json
import os
import re

import numpy as np

from plonky_amd import api, lib
from tests import check_witness_cases as cw
from tests import checked_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "check_witness_refusals.json")


def declarations():
    """{name: (restype, [argtypes], [argument names])} of the header, comments stripped: a pointer is c_void_p, `unsigned` c_uint, `int` c_int"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plonky_hip_witness.h")).read(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"\b(int)\s+(plk_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        types, names = [], []
        for a in args.split(","):
            a = a.strip()
            names.append(a.split()[-1].lstrip("*"))
            types.append(ctypes.c_void_p if "*" in a else {"unsigned": ctypes.c_uint, "int": ctypes.c_int}[a.rsplit(None, 1)[0]])
        out[name] = (ctypes.c_int, types, names)
    return out


def test_header_and_binding_table_agree():
    decl = declarations()
    assert sorted(decl) == sorted(cw.ENTRIES) == sorted(name for name, _, _ in lib.WITNESS_SYMBOLS)
    for name, res, args in lib.WITNESS_SYMBOLS:
        assert res is decl[name][0] and len(args) == len(decl[name][1]) and all(a is b for a, b in zip(args, decl[name][1])), name
    host = ["log_degree", "field", "constants", "constants_stride", "wires", "sigma", "inner_zeta", "inner_a", "report", "row_masks", "first_terms"]
    assert decl["plk_plonk_check_witness"][2] == host == list(cw.ORDER)
    assert decl["plk_plonk_check_witness_dev"][2] == ["log_degree", "field", "d_constants", "constants_stride", "d_wires", "d_sigma", "inner_zeta", "inner_a",
                                                      "d_report", "d_row_masks", "d_first_terms", "stream"]


def test_names_are_apart_from_the_pinned_set():
    pinned = {name for name, _, _ in lib.SYMBOLS}
    assert not pinned & {name for name, _, _ in lib.WITNESS_SYMBOLS}
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plonky_hip.h")).read(), flags=re.S)
    assert "check_witness" not in main


def test_entries_are_exported_and_bound():
    lib.build()
    for so in (lib.SO_PATH, checked_child.CHECKED):
        L = ctypes.CDLL(so)
        for name in cw.ENTRIES:
            assert hasattr(L, name), (so, name)
    L = lib.load()
    for name, res, args in lib.WITNESS_SYMBOLS:
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_python_layers_expose_the_functions():
    from plonky_amd import device
    assert callable(api.check_witness) and callable(api.WitnessReport) and callable(device.check_witness_dev)


def test_refusals_launch_nothing():
    """every refusal with its code and text, on a machine without a device too: they come before one is selected"""
    got = [dict(entry=e, case=c, code=rc, text=t) for e, c, rc, t in cw.refusal_results(lib.load())]
    assert got == json.load(open(GOLDEN))
    texts = {}
    for g, (_, _, starts) in zip(got, cw.REFUSALS * 2):
        assert g["code"] == lib.PLK_ERR_INVALID_ARG and g["text"].startswith(starts), g
        texts.setdefault(g["case"], set()).add(g["text"])
    assert all(len(t) == 1 for t in texts.values()), "the two entries refuse in the same words"
    singles = [next(iter(texts[name])) for name, override, _ in cw.REFUSALS if len(override) == 1 and "field" not in override and "log_degree" not in override
               and "constants_stride" not in override]
    assert len(set(singles)) == len(singles) == 5, "each null pointer has a text of its own"


def test_a_good_call_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        return
    L = lib.load()
    buf = np.zeros(9 * 4 * 4 * 8, dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.plk_plonk_check_witness_dev(2, 0, p, 1, p, None, p, p, p, None, None, None) == lib.PLK_ERR_NO_DEVICE
    assert L.plk_plonk_check_witness(2, 0, p, 8, p, None, p, p, p, None, None) == lib.PLK_ERR_NO_DEVICE
