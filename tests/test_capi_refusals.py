"""CPU or GPU: every argument check a C-ABI wrapper makes before its first device call returns the code and the plk_last_error()
text it returned before the wrappers were reworked (tests/golden/capi_refusals.json, recorded by tests/capi_refusal_cases.py).
No case reaches the device, so the pairs are the same with and without one."""
import json
import os

from plonky_amd import lib
from tests import capi_refusal_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_refusals.json")


def test_every_entry_has_a_case_or_a_reason():
    names = [name for name, _, _ in lib.SYMBOLS]
    with_case = {entry for _, entry, _ in cases.CASES}
    assert not with_case & set(cases.EXCLUDED), sorted(with_case & set(cases.EXCLUDED))
    assert sorted(with_case | set(cases.EXCLUDED)) == sorted(names)
    assert all(len(reason) > 10 for reason in cases.EXCLUDED.values())
    ids = [cases.case_id(label, entry) for label, entry, _ in cases.CASES]
    assert len(set(ids)) == len(ids)


def test_refusals_are_what_they_were():
    want = json.load(open(GOLDEN))
    got = cases.run(lib.load())
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    # the list is what it claims to be: refusals and empty calls, nothing that got as far as a device
    assert all(rc in (lib.PLK_OK, lib.PLK_ERR_INVALID_ARG, lib.PLK_ERR_SIZE_MISMATCH, lib.PLK_ERR_NOT_POW2, lib.PLK_ERR_TWO_ADICITY)
               for rc, _ in want.values())
