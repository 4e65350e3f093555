"""CPU-only: what api.check_witness and device.check_witness_dev hand to the C ABI, pinned from outside over the recorder of
abi_recorder.py: the exact C call with the optional outputs null and non-null, bad shapes refused before any call, and the report
decoded into a WitnessReport from what a queued reply wrote.  libplonky_hip.so is never loaded."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from plonky_amd import api, device, lib
from tests.abi_recorder import ANYPTR, H, NULL, OUT, P, _Recorder, call, refused

STREAM = "stream"
ENTRY, ENTRY_DEV = "plk_plonk_check_witness", "plk_plonk_check_witness_dev"


class _Dev(torch.Tensor):
    is_cuda = True


def dev(*shape, dtype=torch.int64):
    return torch.zeros(shape, dtype=dtype).as_subclass(_Dev)


def limbs(*shape, seed=1):
    return (np.arange(int(np.prod(shape)), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)).reshape(shape)


class _Writing(_Recorder):
    """a reply may also hold bytes for a pointer argument: {index: bytes} in `fill`, stored through the pointer the wrapper passed"""

    def __init__(self):
        super().__init__()
        self.fills = []

    def fill(self, values):
        self.fills.append(values)

    def __getattr__(self, name):
        entry = super().__getattr__(name)
        if name == "plk_last_error":
            return entry

        def writing(*args):
            if self.fills:
                for i, data in self.fills.pop(0).items():
                    ctypes.memmove(args[i], data, len(data))
            return entry(*args)

        return writing


@pytest.fixture
def rec(monkeypatch):
    r = _Writing()
    monkeypatch.setattr(api._lib, "load", lambda: r)
    monkeypatch.setattr(device, "_stream", lambda: STREAM)
    return r


def test_check_witness_call(rec):
    zeta, a = limbs(4, seed=2), limbs(4, seed=3)
    for log_degree, stride, with_sigma, masks in itertools.product((0, 2), (1, 8), (False, True), (False, True)):
        n = 1 << log_degree
        k, w = limbs(6, n * stride, 4), limbs(9, n, 4, seed=5)
        sigma = np.arange(6 * n, dtype=np.uint32)[::-1].copy() if with_sigma else None
        want = (ENTRY, log_degree, 1, H(k), stride, H(w), H(sigma, np.uint32) if with_sigma else NULL, H(zeta), H(a), ANYPTR, ANYPTR if masks else NULL, ANYPTR)
        rep = call(rec, want, api.check_witness, 1, n, k, w, sigma, zeta, a, constants_stride=stride, row_masks=masks)
        assert isinstance(rep, api.WitnessReport) and (rep.row_masks is not None) == masks
        assert rep.first_terms.shape == (8, 4) and rep.first_terms.dtype == np.uint64
        if masks:
            assert rep.row_masks.shape == (n,) and rep.row_masks.dtype == np.uint8
    # sigma in any integer dtype, entries above 2^31 included, goes out as uint32 words
    sigma = np.array([0xFFFFFFFF] + [0] * 5, dtype=np.int64)
    call(rec, (ENTRY, 0, 0, ANYPTR, 1, ANYPTR, H(sigma, np.uint32), ANYPTR, ANYPTR, ANYPTR, NULL, ANYPTR), api.check_witness, 0, 1, limbs(6, 1, 4), limbs(9, 1, 4),
         sigma, zeta, a)


def test_check_witness_refuses_bad_shapes_before_any_call(rec):
    zeta, a = limbs(4), limbs(4)
    k, w = limbs(6, 4, 4), limbs(9, 4, 4)
    refused(rec, api.check_witness, 0, 3, limbs(6, 3, 4), limbs(9, 3, 4), None, zeta, a)  # Not a power of two
    refused(rec, api.check_witness, 0, 4, k, w, None, zeta, a, constants_stride=2)
    refused(rec, api.check_witness, 0, 4, k, w, None, None, a)
    refused(rec, api.check_witness, 0, 4, k, w, None, zeta, None)
    for bad in (lambda: api.check_witness(0, 4, limbs(5, 4, 4), w, None, zeta, a), lambda: api.check_witness(0, 4, k, limbs(8, 4, 4), None, zeta, a),
                lambda: api.check_witness(0, 4, k, w, np.arange(23), zeta, a), lambda: api.check_witness(0, 4, k, w, None, limbs(5), a),
                lambda: api.check_witness(0, 4, k, w, None, zeta, a, constants_stride=8)):
        rec.calls = []
        with pytest.raises(ValueError):
            bad()
        assert rec.calls == []


def test_check_witness_decodes_the_report(rec):
    zeta, a = limbs(4), limbs(4)
    n = 8
    k, w = limbs(6, n, 4), limbs(9, n, 4)
    terms, masks = limbs(8, 4, seed=9), np.array([0, 0, 0, 0, 0, 0x85, 0, 0xFF], dtype=np.uint8)
    rec.fill({8: np.array([2, 5, 0x85, 3, 4 * n + 6, 1, 0, 0], dtype=np.uint32).tobytes(), 9: masks.tobytes(), 10: terms.tobytes()})
    rep = api.check_witness(0, n, k, w, np.arange(6 * n), zeta, a, row_masks=True)
    assert (rep.bad_rows, rep.first_row, rep.first_mask, rep.bad_copies, rep.first_copy, rep.sigma_out_of_range) == (2, 5, 0x85, 3, (4, 6), 1)
    assert np.array_equal(rep.first_terms, terms) and np.array_equal(rep.row_masks, masks) and not rep.ok
    assert rep.message() == "5-th gate constraints are not satisfied" == "{}-th gate constraints are not satisfied".format(5)  # plonk.rs:165
    # nothing failed
    rec.fill({8: np.array([0, 0xFFFFFFFF, 0, 0, 0xFFFFFFFF, 0, 0, 0], dtype=np.uint32).tobytes()})
    rep = api.check_witness(0, n, k, w, None, zeta, a)
    assert rep.ok and rep.first_row is None and rep.first_copy is None and rep.message() is None and rep.row_masks is None
    # each part alone makes it fail
    for words in ([1, 0, 1, 0, 0xFFFFFFFF, 0, 0, 0], [0, 0xFFFFFFFF, 0, 1, 0, 0, 0, 0], [0, 0xFFFFFFFF, 0, 0, 0xFFFFFFFF, 1, 0, 0]):
        rec.fill({8: np.array(words, dtype=np.uint32).tobytes()})
        assert not api.check_witness(0, n, k, w, None, zeta, a).ok
    assert api.WitnessReport(n, np.array([1, 0, 1, 1, 0, 0, 0, 0], dtype=np.int32)).first_copy == (0, 0)  # the device form's int32 words
    assert api.WitnessReport(n, np.array([0, -1, 0, 0, -1, 0, 0, 0], dtype=np.int32)).ok
    # a refusal of the library is a ValueError with its text; any other failure lib.check's error
    rec.reply(ENTRY, lib.PLK_ERR_INVALID_ARG, "bad field id 9")
    with pytest.raises(ValueError, match="bad field id 9"):
        api.check_witness(9, n, k, w, None, zeta, a)
    rec.reply(ENTRY, lib.PLK_ERR_NO_DEVICE, "no device")
    with pytest.raises(lib.PlonkyHipError):
        api.check_witness(0, n, k, w, None, zeta, a)


def test_check_witness_dev_call(rec):
    zeta, a = limbs(4, seed=2), limbs(4, seed=3)
    for log_degree, stride, with_sigma, with_masks, with_terms, own_report in itertools.product((0, 3), (1, 8), (False, True), (False, True), (False, True),
                                                                                                 (False, True)):
        n = 1 << log_degree
        k, w = dev(6, n * stride, 4), dev(9, n, 4)
        sigma = dev(6 * n, dtype=torch.int32) if with_sigma else None
        masks = dev(n, dtype=torch.uint8) if with_masks else None
        terms = dev(8, 4) if with_terms else None
        report = dev(8, dtype=torch.int32) if own_report else None
        want = (ENTRY_DEV, log_degree, 1, P(k), stride, P(w), P(sigma) if with_sigma else NULL, H(zeta), H(a), P(report) if own_report else OUT(),
                P(masks) if with_masks else NULL, P(terms) if with_terms else NULL, STREAM)
        got = call(rec, want, device.check_witness_dev, 1, log_degree, k, w, sigma, zeta, a, constants_stride=stride, report=report, row_masks=masks,
                   first_terms=terms)
        assert (got is report) if own_report else (got.shape == (8,) and got.dtype == torch.int32)
    # the default stride takes constants_8n as it is
    call(rec, (ENTRY_DEV, 2, 0, ANYPTR, 8, ANYPTR, NULL, ANYPTR, ANYPTR, ANYPTR, NULL, NULL, STREAM), device.check_witness_dev, 0, 2, dev(6, 32, 4), dev(9, 4, 4),
         None, zeta, a)


def test_check_witness_dev_refuses_bad_tensors_before_any_call(rec):
    zeta, a = limbs(4), limbs(4)
    good = dict(constants=dev(6, 32, 4), wires=dev(9, 4, 4), sigma=dev(24, dtype=torch.int32), report=dev(8, dtype=torch.int32),
                row_masks=dev(4, dtype=torch.uint8), first_terms=dev(8, 4))

    def attempt(**over):
        kw = dict(good, **over)
        return lambda: device.check_witness_dev(0, 2, kw.pop("constants"), kw.pop("wires"), kw.pop("sigma"), zeta, a, **kw)

    strided = dev(9, 4, 8)[..., ::2]
    bad = dict(constants=[torch.zeros(6, 32, 4, dtype=torch.int64), dev(6, 4, 4), dev(6, 32, 4, dtype=torch.int32)],
               wires=[torch.zeros(9, 4, 4, dtype=torch.int64), dev(6, 4, 4), strided],
               sigma=[dev(24), dev(23, dtype=torch.int32), torch.zeros(24, dtype=torch.int32)],
               report=[dev(8), dev(7, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)],
               row_masks=[dev(4), dev(5, dtype=torch.uint8), dev(1, 4, dtype=torch.uint8)],
               first_terms=[dev(8, 4, dtype=torch.int32), dev(4, 8), dev(32)])
    for name, tensors in bad.items():
        for t in tensors:
            refused(rec, attempt(**{name: t}))
    refused(rec, attempt(constants_stride=4))
    refused(rec, lambda: device.check_witness_dev(0, 2, good["constants"], good["wires"], None, None, a))
    refused(rec, lambda: device.check_witness_dev(0, 2, good["constants"], good["wires"], None, zeta, None))
