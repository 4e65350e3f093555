"""CPU-only: the case table of tests/sqrt_cases.py against itself and against the oracle, on all six fields.  The table is what
test_fe_sqrt_host_replay.py and test_gpu_field_utils.py feed to fe_sqrt / fe_sqrt_tabled, so what it claims about every input - the
depths the loop walks, which inputs have no root, which of the two roots the reference returns - is checked here first."""
import pytest

from oracle import oracle_lib as ol
from tests import sqrt_cases as sc
from tests.util import ints_to_array, limbs_to_int


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    ol.build()


@pytest.mark.parametrize("f", sc.FIELDS, ids=lambda f: f.name)
def test_the_table_reaches_every_depth_and_every_exit(f):
    A = f.two_adicity
    cases = sc.build_cases(f)
    assert cases == sc.build_cases(f)  # the same table for every user
    by = {label: ks for label, _, ks in cases}
    for k in range(1, A):
        assert by["one_step_k%d_h0" % k] == [k]
        assert by["descend_from_k%d_h0" % k] == list(range(k, 0, -1))
    assert by["two_to_A_minus_2_h0"] == [A - 1] and by["b_is_one_h0"] == [] and by["zero"] == [] and by["one"] == []
    assert by["minus_one"] == [1]  # -1 = zeta^(2^(A-1))
    assert by["generator"] is None and sum(ks is None for ks in by.values()) >= 5 * sc.H_PER_CASE + 1
    for label in ("alt_5555_h0", "alt_aaaa_h0"):
        ks = by[label]
        assert len(ks) >= A // 2 - 1 and ks == sorted(ks, reverse=True) and len(set(ks)) == len(ks)
    assert len({a for _, a, _ in cases}) >= len(cases) - 2  # three different h give three different inputs


@pytest.mark.parametrize("f", sc.FIELDS, ids=lambda f: f.name)
def test_restatement_walks_the_intended_depths_and_agrees_with_the_oracle(f):
    for label, a, want_ks in sc.build_cases(f):
        root, ks = sc.restated_sqrt(f, a)
        got = ol.field_sqrt(f.field_id, ints_to_array([f.to_mont(a)], f.n_limbs))
        if want_ks is None:
            assert root is None and got is None, label
            continue
        assert ks == want_ks, label
        assert root * root % f.p == a, label
        assert got is not None and limbs_to_int(got[0]) == f.to_mont(root), label  # the same one of the two roots, limb for limb
