"""CPU-only: the ten Rescue entries (plk_rescue_create / _free / _rounds / _mds, plk_rescue_permutation[_dev], plk_rescue_sponge[_dev],
plk_field_kth_root[_dev]) are declared in include/plonky_hip.h with the argument lists INTEGRATION.md gives - a count or the width
first, context or field id second: the id-first entries are a pinned set (tests/test_gpu_dispatch_ids.py) - bound in lib.SYMBOLS,
exported by libplonky_hip.so and its checked twin, and wrapped by api / device.  The restatement tests/rescue_ref.py is held to what integers alone can say about it."""
import ctypes
import os
import re

import pytest

from oracle import bigint_ref as br
from plonky_amd import api, lib
from tests import checked_child
from tests import rescue_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CTX = r"const\s+plk_rescue_ctx\s*\*\s*ctx"
DECLARATIONS = {
    "plk_rescue_create": r"size_t\s+width\s*,\s*int\s+field\s*,\s*size_t\s+rounds\s*,\s*const\s+uint64_t\s*\*\s*constants\s*,\s*plk_rescue_ctx\s*\*\*\s*out",
    "plk_rescue_free": r"plk_rescue_ctx\s*\*\s*ctx",
    "plk_rescue_rounds": r"size_t\s+width\s*,\s*size_t\s+security_bits\s*,\s*size_t\s*\*\s*rounds",
    "plk_rescue_mds": r"size_t\s+width\s*,\s*int\s+field\s*,\s*uint64_t\s*\*\s*out",
    "plk_rescue_permutation": r"size_t\s+count\s*,\s*" + _CTX + r"\s*,\s*const\s+uint64_t\s*\*\s*states\s*,\s*uint64_t\s*\*\s*out",
    "plk_rescue_permutation_dev": r"size_t\s+count\s*,\s*" + _CTX + r"\s*,\s*const\s+void\s*\*\s*d_states\s*,\s*void\s*\*\s*d_out\s*,\s*void\s*\*\s*stream",
    "plk_rescue_sponge": r"size_t\s+count\s*,\s*" + _CTX + r"\s*,\s*size_t\s+n_inputs\s*,\s*const\s+uint64_t\s*\*\s*inputs\s*,\s*size_t\s+n_outputs\s*,\s*uint64_t\s*\*\s*out",
    "plk_rescue_sponge_dev": r"size_t\s+count\s*,\s*" + _CTX + r"\s*,\s*size_t\s+n_inputs\s*,\s*const\s+void\s*\*\s*d_inputs\s*,\s*size_t\s+n_outputs\s*,"
                             r"\s*void\s*\*\s*d_out\s*,\s*void\s*\*\s*stream",
    "plk_field_kth_root": r"size_t\s+count\s*,\s*int\s+field\s*,\s*uint32_t\s+k\s*,\s*const\s+uint64_t\s*\*\s*in\s*,\s*uint64_t\s*\*\s*out",
    "plk_field_kth_root_dev": r"size_t\s+count\s*,\s*int\s+field\s*,\s*uint32_t\s+k\s*,\s*const\s+void\s*\*\s*d_in\s*,\s*void\s*\*\s*d_out\s*,\s*void\s*\*\s*stream",
}
N_ARGS = {"plk_rescue_create": 5, "plk_rescue_free": 1, "plk_rescue_rounds": 3, "plk_rescue_mds": 3, "plk_rescue_permutation": 4,
          "plk_rescue_permutation_dev": 5, "plk_rescue_sponge": 6, "plk_rescue_sponge_dev": 7, "plk_field_kth_root": 5, "plk_field_kth_root_dev": 6}
COUNT_FIRST = [n for n in DECLARATIONS if n != "plk_rescue_free"]  # a count or a size first: none joins the pinned id-first set


def test_entries_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plonky_hip.h")).read(), flags=re.S)
    bound = {name: args for name, _, args in lib.SYMBOLS}
    assert len(DECLARATIONS) == 10
    for name, args in DECLARATIONS.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text), name
        assert name in bound and len(bound[name]) == N_ARGS[name], name
    for name in COUNT_FIRST:
        assert bound[name][0] is ctypes.c_size_t, name
    assert bound["plk_rescue_create"][1] is ctypes.c_int and bound["plk_rescue_mds"][1] is ctypes.c_int
    for name in ("plk_field_kth_root", "plk_field_kth_root_dev"):
        assert bound[name][1] is ctypes.c_int and bound[name][2] is ctypes.c_uint32, name
    assert re.search(r"typedef\s+struct\s+plk_rescue_ctx\s+plk_rescue_ctx\s*;", text)


def test_entries_are_exported_by_both_builds():
    lib.build()
    for so in (lib.SO_PATH, checked_child.CHECKED):
        L = ctypes.CDLL(so)
        for name in DECLARATIONS:
            assert hasattr(L, name), (so, name)


def test_python_layers_expose_the_reference_names():
    from plonky_amd import device
    for name in ("rescue_rounds", "rescue_mds", "RescueContext", "rescue_permutation", "rescue_sponge", "rescue_hash_n_to_1", "rescue_hash_n_to_2",
                 "rescue_hash_n_to_3", "kth_root", "Challenger"):
        assert callable(getattr(api, name)), name
    for name in ("observe_element", "observe_elements", "observe_affine_point", "observe_affine_points", "get_challenge", "get_2_challenges",
                 "get_3_challenges", "get_n_challenges", "clone"):
        assert callable(getattr(api.Challenger, name)), name
    for name in ("__enter__", "__exit__", "free"):
        assert callable(getattr(api.RescueContext, name)), name
    for name in ("rescue_permutation_dev", "rescue_sponge_dev", "kth_root_dev"):
        assert callable(getattr(device, name)), name


# ---- the restatement against itself, where integers allow ----
@pytest.mark.parametrize("field", sorted(br.FIELDS))
def test_ref_kth_root_inverts_the_power(field):
    f = br.FIELDS[field]
    from math import gcd
    xs = [0, 1, f.p - 1, 2] + [br.limbs_to_int(l) for l in br.rand_field_limbs(f, 5, 4)]
    for k in (1, 3, 5, 7, 11, 13):
        d = rr.kth_root_exponent(f.p, k)
        assert (d is None) == (gcd(k, f.p - 1) != 1), k
        if d is not None:
            for x in xs:
                assert pow(rr.kth_root(f.p, x, k), k, f.p) == x
    assert rr.kth_root_exponent(f.p, rr.ALPHA[field]) is not None
    assert rr.kth_root_exponent(f.p, 3) is None
    # ALPHA is the first of 5 and 11 that permutes the field: 11 on Bls12377Scalar alone
    assert rr.ALPHA[field] == (5 if gcd(5, f.p - 1) == 1 else 11)
    permuting = {k for k in (5, 7, 11, 13) if gcd(k, f.p - 1) == 1}
    assert permuting == ({11} if field == 2 else {5, 11} if field == 3 else {5, 7, 11, 13})


@pytest.mark.parametrize("field", sorted(br.FIELDS))
def test_ref_mds_matrix_is_invertible_and_cauchy(field):
    p = br.FIELDS[field].p
    m = rr.mds_matrix(p, 4)
    for r in range(4):
        for c in range(4):
            assert m[r][c] * (4 + r - c) % p == 1
    # Gauss-Jordan over the field: M * M^-1 = I
    n = 4
    a = [row[:] + [1 if i == j else 0 for j in range(n)] for i, row in enumerate(m)]
    for col in range(n):
        piv = next(r for r in range(col, n) if a[r][col])
        a[col], a[piv] = a[piv], a[col]
        inv = pow(a[col][col], -1, p)
        a[col] = [v * inv % p for v in a[col]]
        for r in range(n):
            if r != col and a[r][col]:
                a[r] = [(v - a[r][col] * w) % p for v, w in zip(a[r], a[col])]
    minv = [row[n:] for row in a]
    for r in range(n):
        for c in range(n):
            assert sum(m[r][k] * minv[k][c] for k in range(n)) % p == (1 if r == c else 0)
    x = [3, 1, 4, 1]
    assert rr.apply_mds(p, x) == [sum(m[r][c] * x[c] for c in range(4)) % p for r in range(4)]


def test_ref_rounds():
    assert rr.recommended_rounds(4, 128) == 16 and rr.recommended_rounds(4, 64) == 10
    assert rr.recommended_rounds(4, 129) == 17 and rr.recommended_rounds(3, 128) == 22


def test_ref_sponge_and_challenger_shapes():
    field = 0
    consts = rr.constants(field, 4, 2)
    assert len(consts) == 2 and all(len(a) == 4 and len(b) == 4 for a, b in consts)
    # no input: no permutation before the first squeeze, so the first three outputs are the zero state
    assert rr.rescue_sponge(field, [], 3, consts) == [0, 0, 0]
    four = rr.rescue_sponge(field, [], 4, consts)
    assert four[:3] == [0, 0, 0] and four[3] == rr.rescue_permutation(field, [0] * 4, consts)[0]
    # a short last chunk adds fewer elements: [a, b, c, d] is two permutations
    s1 = rr.rescue_permutation(field, [1, 2, 3, 0], consts)
    s2 = rr.rescue_permutation(field, [(s1[0] + 4) % br.FIELDS[field].p] + s1[1:], consts)
    assert rr.rescue_sponge(field, [1, 2, 3, 4], 2, consts) == s2[:2]
    # the Challenger pops from the end, and repeats itself when nothing is observed in between
    c = rr.Challenger(field, consts)
    c.observe_elements([1, 2, 3])
    assert c.get_challenge() == s1[2]
    assert c.get_2_challenges() == (s1[2], s1[2])
    d = c.clone()
    d.observe_element(9)
    assert d.get_challenge() != s1[2] and c.get_challenge() == s1[2]
