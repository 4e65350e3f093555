"""CPU-only: the four gate-trace entries (plk_trace_rescue_permutation[_dev], plk_trace_curve_msm[_dev]) are declared in a header of
their own, include/plonky_hip_trace.h, count first; lib.TRACE_SYMBOLS binds exactly what that header declares, apart from lib.SYMBOLS
(which mirrors include/plonky_hip.h) and lib.WITNESS_SYMBOLS; both libraries export them; every refusal that needs no context comes
back with its code and its documented text, in the documented order, before a device is selected; the Python wrappers make exactly
the C call the header describes (tests/abi_recorder.py) and make none when their own checks refuse."""
import ctypes
import os
import re

import numpy as np
import pytest

from plonky_amd import api, lib
from tests import checked_child
from tests import gate_trace_cases as gc
from tests.abi_recorder import ANYPTR, H, HND, NULL, _Recorder, call, refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"unsigned": ctypes.c_uint, "int": ctypes.c_int, "size_t": ctypes.c_size_t}


def declarations():
    """{name: ([argtypes], [argument names])} of the header, comments stripped: a pointer is c_void_p"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plonky_hip_trace.h")).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(plk_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        parts = [a.strip() for a in args.split(",")]
        out[name] = ([ctypes.c_void_p if "*" in a else CTYPES[a.rsplit(None, 1)[0]] for a in parts], [a.split()[-1].lstrip("*") for a in parts])
    return out


def test_header_and_binding_table_agree():
    decl = declarations()
    assert sorted(decl) == sorted(gc.ENTRIES) == sorted(name for name, _, _ in lib.TRACE_SYMBOLS)
    for name, res, args in lib.TRACE_SYMBOLS:
        assert res is ctypes.c_int and len(args) == len(decl[name][0]) and all(a is b for a, b in zip(args, decl[name][0])), name
    assert decl["plk_trace_rescue_permutation"][1] == list(gc.RESCUE_ORDER)
    assert decl["plk_trace_curve_msm"][1] == list(gc.MSM_ORDER)
    for host, dev in (("plk_trace_rescue_permutation", "plk_trace_rescue_permutation_dev"), ("plk_trace_curve_msm", "plk_trace_curve_msm_dev")):
        want = [n if n in ("count", "ctx", "parts", "n_bits", "curve", "n_rows", "start_xy") else "d_" + n for n in decl[host][1]] + ["stream"]
        assert decl[dev][1] == want, dev
        assert decl[dev][0][0] is ctypes.c_size_t  # a count first: none joins the pinned id-first set


def test_names_are_apart_from_the_pinned_sets():
    trace = {name for name, _, _ in lib.TRACE_SYMBOLS}
    assert not trace & {name for name, _, _ in lib.SYMBOLS} and not trace & {name for name, _, _ in lib.WITNESS_SYMBOLS}
    for header in ("plonky_hip.h", "plonky_hip_witness.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        assert "plk_trace" not in text, header


def test_entries_are_exported_and_bound():
    lib.build()
    for so in (lib.SO_PATH, checked_child.CHECKED):
        L = ctypes.CDLL(so)
        for name in gc.ENTRIES:
            assert hasattr(L, name), (so, name)
    L = lib.load()
    for name, res, args in lib.TRACE_SYMBOLS:
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_python_layers_expose_the_functions():
    from plonky_amd import device
    for name in ("trace_rescue_permutation", "trace_curve_msm"):
        assert callable(getattr(api, name)) and callable(getattr(device, name + "_dev")), name


def test_refusals_launch_nothing():
    """every refusal that needs no context, through both forms, on a machine without a device too: they come before one is selected
    (a device would answer a good call; without one it is PLK_ERR_NO_DEVICE, which no refusal is)"""
    L = lib.load()
    got = gc.refusal_results(L, gc.ENTRIES[2:], gc.MSM_ORDER, gc.MSM_GOOD, gc.MSM_REFUSALS)
    got += gc.refusal_results(L, gc.ENTRIES[:2], gc.RESCUE_ORDER, gc.RESCUE_GOOD, gc.RESCUE_REFUSALS[:2])
    want = [(e, r) for e in gc.ENTRIES[2:] for r in gc.MSM_REFUSALS] + [(e, r) for e in gc.ENTRIES[:2] for r in gc.RESCUE_REFUSALS[:2]]
    assert len(got) == len(want)
    texts = {}
    for (entry, name, code, text), (e, (n, _, starts)) in zip(got, want):
        assert (entry, name) == (e, n) and code == lib.PLK_ERR_INVALID_ARG and text.startswith(starts), (entry, name, code, text)
        texts.setdefault((entry.replace("_dev", ""), name), set()).add(text)
    assert all(len(t) == 1 for t in texts.values()), "the two forms refuse in the same words"


def test_count_zero_is_ok_and_a_good_call_fails_loudly_without_a_gpu():
    L = lib.load()
    buf = np.zeros(9 * 64 * 4, dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.plk_trace_curve_msm_dev(0, 2, 8, 0, None, None, p, 64, None, None, None, None, None) == lib.PLK_OK
    assert L.plk_trace_curve_msm(0, 2, 8, 0, None, None, p, 64, None, None, None, None) == lib.PLK_OK
    import torch
    if torch.cuda.is_available():
        return
    assert L.plk_trace_curve_msm_dev(1, 2, 8, 0, p, p, p, 64, p, p, None, None, None) == lib.PLK_ERR_NO_DEVICE
    assert L.plk_trace_curve_msm(1, 2, 8, 0, p, p, p, 64, p, p, None, None) == lib.PLK_ERR_NO_DEVICE


# ---- the Python wrappers over the recorder: the C call they make, and none when they refuse ----
class _Ctx:
    field, width, rounds = 0, 4, 2
    handle = ctypes.c_void_p(0x7ACE)


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(api._lib, "load", lambda: r)
    return r


def test_api_trace_rescue_permutation_call(rec):
    inputs = np.arange(3 * 4 * 4, dtype=np.uint64).reshape(3, 4, 4)
    first = [0, 5, 10]
    want = ("plk_trace_rescue_permutation", 3, HND(0x7ACE), H(inputs), 16, ANYPTR, H(first, np.uint32), NULL, ANYPTR)
    w, k, st = call(rec, want, api.trace_rescue_permutation, _Ctx, inputs, 16, first)
    assert w.shape == (9, 16, 4) and not w.any() and k is None and st.shape == (4,) and st.dtype == np.uint32
    mine = np.ones((9, 16, 4), dtype=np.uint64)
    want = ("plk_trace_rescue_permutation", 3, HND(0x7ACE), H(inputs), 16, ("ptr", mine.ctypes.data), H(first, np.uint32), ANYPTR, ANYPTR)
    w, k, _ = call(rec, want, api.trace_rescue_permutation, _Ctx, inputs, 16, first, wires=mine, constants=True)
    assert np.shares_memory(w, mine) and k.shape == (6, 16, 4)
    refused(rec, api.trace_rescue_permutation, _Ctx, inputs[:, :3], 16, first)          # states of three elements
    refused(rec, api.trace_rescue_permutation, _Ctx, inputs, 16, first, wires=mine[:8])  # a table of eight wires
    rec.reply("plk_trace_rescue_permutation", rc=lib.PLK_ERR_INVALID_ARG, error="n_rows 0: a table has 1 .. 2^27 rows")
    with pytest.raises(ValueError, match="n_rows 0"):
        api.trace_rescue_permutation(_Ctx, inputs, 16, first)


def test_api_trace_curve_msm_call(rec):
    pts = np.arange(2 * 3 * 2 * 4, dtype=np.uint64).reshape(2, 3, 2, 4)
    scs = np.arange(2 * 3 * 4, dtype=np.uint64).reshape(2, 3, 4) + 100
    start = np.arange(8, dtype=np.uint64).reshape(2, 4) + 7
    want = ("plk_trace_curve_msm", 2, 3, 5, 1, H(pts), H(scs), H(start), 64, ANYPTR, H([0, 20], np.uint32), NULL, ANYPTR)
    w, k, st = call(rec, want, api.trace_curve_msm, 1, pts, scs, start, 5, 64, [0, 20])
    assert w.shape == (9, 64, 4) and k is None and st.shape == (4,)
    refused(rec, api.trace_curve_msm, 1, pts[:, :, :1], scs, start, 5, 64, [0, 20])  # points without y
    refused(rec, api.trace_curve_msm, 1, pts, scs[:1], start, 5, 64, [0, 20])        # fewer scalars than points
    for text, exc in (("x_1 = x_2: instance 1, block row 7", AssertionError), ("y = 0: instance 0, block row 2", AssertionError),
                      ("scalar bit at or above n_bits 5: instance 1", ValueError), ("parts 9: a curve_msm block takes 1 .. 8 parts", ValueError)):
        rec.reply("plk_trace_curve_msm", rc=lib.PLK_ERR_INVALID_ARG, error=text)
        with pytest.raises(exc, match=re.escape(text[:9])):
            api.trace_curve_msm(1, pts, scs, start, 5, 64, [0, 20])
