"""CPU-only: the sigma entries (plk_plonk_sigma[_dev]) are declared in include/plonky_hip.h size first, bound in lib.SYMBOLS, exported by
both libraries and refuse bad arguments before anything is launched; the host mirror api.TargetPartitions / api.WirePartitions
agrees with the restatement of partition.rs in tests/partition_ref.py on seeded merge sequences, and its to_csr with its to_sigma."""
import ctypes
import os
import re

import numpy as np
import pytest

from plonky_amd import api, lib
from tests import checked_child
from tests import partition_ref as pref
from tests import sigma_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, I, P, Z = ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
SIGNATURES = {
    "plk_plonk_sigma_dev": [U, I, P, P, Z, Z, P, P, P, P, P],
    "plk_plonk_sigma": [U, I, P, P, Z, P, P, P],
}


def test_entries_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plonky_hip.h")).read(), flags=re.S)
    bound = {name: (res, args) for name, res, args in lib.SYMBOLS}
    for name, args in SIGNATURES.items():
        assert re.search(r"\bint\s+%s\s*\(\s*unsigned\s+log_degree\s*,\s*int\s+field\b" % name, text), name
        assert name in bound and bound[name][0] is I, name
        assert len(bound[name][1]) == len(args) and all(a is b for a, b in zip(bound[name][1], args)), name
    decl = re.search(r"plk_plonk_sigma_dev\s*\(([^)]*)\)", text).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["log_degree", "field", "d_members", "d_offsets", "num_partitions", "num_members", "k_is",
                                                                    "d_sigma", "d_s_sigma", "d_status", "stream"]


def test_entries_are_exported():
    lib.build()
    for so in (lib.SO_PATH, checked_child.CHECKED):
        L = ctypes.CDLL(so)
        for name in SIGNATURES:
            assert hasattr(L, name), (so, name)


def test_python_layers_expose_the_functions():
    from plonky_amd import device
    for name in ("TargetPartitions", "WirePartitions", "sigma_polynomials", "wire_partitions_to_sigma"):
        assert callable(getattr(api, name)), name
    for name in ("sigma_dev", "circuit_key_dev"):
        assert callable(getattr(device, name)), name


def test_argument_errors_launch_nothing():
    """unknown field ids, a null k_is, log_degree > 27 (and the other refusals) come back with PLK_ERR_INVALID_ARG and their text before a
    device is selected: they do so on a machine without one"""
    L = lib.load()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.c_void_p)

    def err(rc):
        assert rc == lib.PLK_ERR_INVALID_ARG, rc
        return L.plk_last_error().decode()

    for field in (-1, 3, 6, 1000):  # 3: the 6-limb base field of BLS12-377
        assert err(L.plk_plonk_sigma_dev(2, field, p, p, 1, 1, p, p, p, None, None)).startswith("field %d is not a circuit scalar field" % field)
        assert err(L.plk_plonk_sigma(2, field, p, p, 1, p, p, p)).startswith("field %d is not a circuit scalar field" % field)
    assert err(L.plk_plonk_sigma_dev(2, 0, p, p, 1, 1, None, p, p, None, None)).startswith("null k_is")
    assert err(L.plk_plonk_sigma(2, 0, p, p, 1, None, p, p)).startswith("null k_is")
    assert err(L.plk_plonk_sigma_dev(28, 0, p, p, 1, 1, p, p, p, None, None)).startswith("log_degree 28")
    assert err(L.plk_plonk_sigma(28, 0, p, p, 1, p, p, p)).startswith("log_degree 28")
    assert err(L.plk_plonk_sigma_dev(2, 0, p, p, 1, 1, p, None, None, None, None)).startswith("neither d_sigma nor d_s_sigma")
    assert err(L.plk_plonk_sigma(2, 0, p, p, 1, p, None, None)).startswith("neither sigma nor s_sigma")
    assert err(L.plk_plonk_sigma_dev(2, 0, p, None, 1, 1, p, p, p, None, None)).startswith("null device pointer")
    assert err(L.plk_plonk_sigma_dev(2, 0, p, p, 0, 1, p, p, p, None, None)).startswith("1 members in no partition")
    # the host form looks at offsets itself: a start that is not 0, a decrease
    off = np.array([1, 2, 3], dtype=np.uint32)
    assert err(L.plk_plonk_sigma(2, 0, p, off.ctypes.data_as(P), 2, p, p, p)).startswith("offsets[0] is 1")
    off = np.array([0, 3, 2], dtype=np.uint32)
    assert err(L.plk_plonk_sigma(2, 0, p, off.ctypes.data_as(P), 2, p, p, p)).startswith("offsets decrease at partition 1")


def both(n, ops, n_virtual):
    return sc.build_partitions(api.TargetPartitions, n, ops, n_virtual), sc.build_partitions(pref.TargetPartitionsRef, n, ops, n_virtual)


def sequences(n):
    w = lambda g, i: ("wire", g, i)
    v = lambda k: ("virtual", k)
    return {
        "repeated merges of one pair": [(w(0, 0), w(1, 1))] * 3 + [(w(1, 1), w(0, 0))] * 2,
        "into a merged class from either side": [(w(0, 0), w(1, 0)), (w(2, 0), w(0, 0)), (w(1, 0), w(3, 1)), (w(3, 2), w(2, 0)), (w(0, 0), w(3, 2))],
        "virtual bridges": [(w(0, 1), v(0)), (v(0), w(2, 3)), (v(1), w(1, 1)), (w(3, 5), v(1)), (v(0), v(1))],
        "stale lists": [(w(0, 0), w(0, 1)), (w(0, 1), w(0, 2)), (w(0, 2), w(0, 3)), (w(1, 4), w(0, 0)), (w(0, 3), w(2, 5))],
        "seeded": sc.merge_sequence(n, 0x5E0 + n, n_virtual=4, n_merges=6 * n),
        "seeded, capped": sc.merge_sequence(n, 0x5E1 + n, n_virtual=4, n_merges=6 * n, cap=3),
    }


@pytest.mark.parametrize("n", [4, 16])
def test_mirror_equals_the_restated_reference(n):
    for name, ops in sequences(n).items():
        mine, ref = both(n, ops, 4)
        assert mine.partitions == ref.partitions and mine.indices == ref.indices, name  # stale lists included
        if name == "stale lists":
            pointed = set(ref.indices.values())
            assert any(q not in pointed and len(part) > 1 for q, part in enumerate(ref.partitions)), "no stale list of more than one member"
        wm, wr = mine.to_wire_partitions(), ref.to_wire_partitions()
        assert wm.partitions == wr.partitions and wm.indices == wr.indices, name
        assert wm.to_sigma() == wr.to_sigma(), name


@pytest.mark.parametrize("n", [4, 16])
def test_to_csr_and_the_neighbour_rule_give_to_sigma(n):
    for name, ops in sequences(n).items():
        wp = sc.build_partitions(api.TargetPartitions, n, ops, 4).to_wire_partitions()
        members, offsets = wp.to_csr(n)
        assert members.dtype == np.uint32 and offsets.dtype == np.uint32 and offsets[0] == 0 and offsets[-1] == members.shape[0] == 9 * n
        assert np.all(np.diff(offsets.astype(np.int64)) >= 1), "only live partitions are emitted, and a live one holds a wire"
        assert sorted(members.tolist()) == list(range(9 * n)), name  # the stale lists would list wires twice
        assert sc.neighbour_rule(members, offsets, n).tolist() == wp.to_sigma(), name


def test_mirror_refuses_a_non_routed_wire_in_company():
    tp = sc.build_partitions(api.TargetPartitions, 4, [(("wire", 0, 7), ("wire", 1, 0))], 0)
    with pytest.raises(AssertionError, match="Non-routed wires"):
        tp.to_wire_partitions()
