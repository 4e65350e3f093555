"""CPU-only: the case table of the structured-input NTT tests (tests/ntt_structured_cases.py) is what it says it is.

The GPU test holds k_ntt_pass to the oracle's output and, where the table gives one, to a closed form.  Here every closed form is
recomputed twice from the case's own input - by bigint_ref.ntt / intt on the canonical values and, limb for limb, by the oracle's
C++ restatement of the reference (fft_with_precomputation_power_of_2 and its inverse) on the Montgomery words - the vectors that are
gathered from the power table are rebuilt value by value, the raw-word patterns are checked to be field elements, and the kinds the
table promises are counted so that a later edit cannot thin one out unnoticed.

Zero padding: the GPU test expects of a padded transform the oracle's power-of-two transform of the input followed by zeros.  The
reference's fft_with_precomputation (fft.rs:60-80) pads to the next power of two of the input's own length n', so for a length above
n / 2 the two are the same call; for a shorter one its n' outputs are every (n / n')-th entry of the expectation (w_n^(n / n') is the
primitive n'-th root), and bigint_ref.ntt of the padded values pins the entries in between."""
import numpy as np
import pytest

from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from tests import ntt_structured_cases as nsc
from tests.test_oracle_kats import from_mont_arr, mont_arr

FIELDS = [br.TWEEDLEDEE_BASE, br.BLS12_377_SCALAR, br.BLS12_377_BASE]
LOG_NS = [1, 2, 5, 8]


@pytest.mark.parametrize("f", list(br.FIELDS.values()), ids=lambda f: f.name)
def test_raw_patterns_are_field_elements(f):
    pats = nsc.raw_patterns(f)
    b = f.p.bit_length()
    assert len({n for n, _ in pats}) == len(pats) and len({w for _, w in pats}) == len(pats)
    assert all(0 <= w < f.p for _, w in pats)
    words = dict(pats)
    nz = -(-b // nsc.LIMB_BITS)  # the 29-bit limbs a value below p can reach: 9 (13 for Bls12377Base)
    assert nz == {255: 9, 253: 9, 377: 13}[b]
    for j in range(1, nz + 1):  # every limb boundary below p, from both sides, and none above
        if 1 << (29 * j) < f.p:
            assert words["2^%d" % (29 * j)] == 1 << (29 * j) and words["2^%d-1" % (29 * j)] == (1 << (29 * j)) - 1
        else:
            assert j == nz and "2^%d" % (29 * j) not in words and "2^%d-1" % (29 * j) not in words
    assert words["2^(b-1)-1"].bit_length() == b - 1 and words["2^(b-1)-1"] & (words["2^(b-1)-1"] + 1) == 0
    limbs = [(words["alt-limbs"] >> (29 * j)) & ((1 << 29) - 1) for j in range(nz)]
    assert all(l == 0 for l in limbs[0::2]) and all(l == (1 << 29) - 1 for l in limbs[1:-1:2]) and words["alt-limbs"] < 1 << (b - 1)
    cyc = nsc.pattern_cycle(f, 3 * len(pats) + 1)
    assert nsc._ints(cyc) == [w for _, w in pats] * 3 + [pats[0][1]]


@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
@pytest.mark.parametrize("log_n", LOG_NS)
def test_table_holds_what_it_promises(f, log_n):
    n, p = 1 << log_n, f.p
    cs = nsc.cases(f.field_id, log_n)
    names = [c.name for c in cs]
    want = ["zero", "alternating", "half_zero_tail", "half_zero_head", "raw_cycle", "constant(1)", "constant(p-1)"]
    for i in sorted({0, 1, n // 2, n - 1}):
        want += ["delta(%s,%s)" % (nsc._index_name(i, n), v) for v in ("1", "p-1")]
    for m in sorted({1, n // 2, n - 1}):
        want += ["geometric(%s,%s)" % (nsc._index_name(m, n), v) for v in ("1", "p-1")]
    for name, _ in nsc.raw_patterns(f):
        want += ["raw_constant(%s)" % name, "raw_delta(0,%s)" % name]
    assert sorted(names) == sorted(want)
    w = f.primitive_root_of_unity(log_n)
    for c in cs:
        assert c.x.shape == (n, f.n_limbs) and c.x.dtype == np.uint64
        vals = c.values()
        assert all(0 <= v < p for v in vals)
        assert np.array_equal(c.x, mont_arr(f, vals)) and from_mont_arr(f, c.x) == vals, c.name
    # the definitions, from the literal values
    assert nsc.case(f.field_id, log_n, "alternating").values() == [1, p - 1] * (n // 2)
    assert nsc.case(f.field_id, log_n, "delta(0,p-1)").values() == [p - 1] + [0] * (n - 1)
    assert nsc.case(f.field_id, log_n, "constant(p-1)").values() == [p - 1] * n
    for m, tag in [(1, "1"), (n // 2, nsc._index_name(n // 2, n)), (n - 1, nsc._index_name(n - 1, n))]:
        for c, ctag in [(1, "1"), (p - 1, "p-1")]:
            assert nsc.case(f.field_id, log_n, "geometric(%s,%s)" % (tag, ctag)).values() == [c * pow(w, -m * k, p) % p for k in range(n)]
    tail, head = nsc.case(f.field_id, log_n, "half_zero_tail").x, nsc.case(f.field_id, log_n, "half_zero_head").x
    assert not tail[n // 2:].any() and not head[: n // 2].any() and tail[: n // 2].any(axis=1).all() and head[n // 2:].any(axis=1).all()
    for name, words in nsc.raw_patterns(f):
        assert nsc._ints(nsc.case(f.field_id, log_n, "raw_constant(%s)" % name).x) == [words] * n
        assert nsc._ints(nsc.case(f.field_id, log_n, "raw_delta(0,%s)" % name).x) == [words] + [0] * (n - 1)


@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
@pytest.mark.parametrize("log_n", LOG_NS)
def test_closed_forms_match_big_integers_and_the_oracle(f, log_n):
    n = 1 << log_n
    opre = ol.FftPrecomputation(f.field_id, n)
    closed = 0
    for c in nsc.cases(f.field_id, log_n):
        vals = c.values()
        big_fwd, big_inv = br.ntt(f, vals), br.intt(f, vals)
        orc_fwd = opre.fft_with_precomputation_power_of_2(c.x)
        orc_inv = opre.ifft_with_precomputation_power_of_2(c.x)
        # the two references agree on every case, closed form or not
        assert np.array_equal(orc_fwd, mont_arr(f, big_fwd)) and np.array_equal(orc_inv, mont_arr(f, big_inv)), c.name
        assert (c.fwd is None) == (c.inv is None)
        if c.fwd is not None:
            closed += 1
            fwd, inv = c.fwd(), c.inv()
            assert fwd == big_fwd and inv == big_inv, c.name
            assert np.array_equal(mont_arr(f, fwd), orc_fwd) and np.array_equal(mont_arr(f, inv), orc_inv), c.name
    assert closed == len(nsc.cases(f.field_id, log_n)) - 4  # alternating, the two half-zero vectors and the pattern cycle have none


def test_closed_form_shapes():
    """the sparse closed forms are sparse where the table says so: exact zeros, one entry"""
    f, log_n = br.TWEEDLEDEE_BASE, 5
    n, p = 32, f.p
    assert nsc.case(0, log_n, "constant(p-1)").fwd() == [n * (p - 1) % p] + [0] * (n - 1)
    assert nsc.case(0, log_n, "constant(p-1)").inv() == [p - 1] + [0] * (n - 1)
    g = nsc.case(0, log_n, "geometric(1,1)")
    assert g.fwd() == [0, n] + [0] * (n - 2) and g.inv() == [0] * (n - 1) + [1]
    assert nsc.case(0, log_n, "delta(0,p-1)").fwd() == [p - 1] * n
    assert nsc.case(0, log_n, "zero").fwd() == [0] * n


PADDED_LOG_N = 8
PADDED_FIRST = [8, 3, 6, 7]  # the first passes the GPU test runs, scaled to 2^8: one pass, and short / middling / tall first passes


@pytest.mark.parametrize("first", PADDED_FIRST)
def test_padded_lengths_visit_every_skip(first):
    lens = nsc.padded_lengths(PADDED_LOG_N, first)
    n = 1 << PADDED_LOG_N
    assert {0, 1, 2, 3, n - 1, n} <= set(lens) and all(0 <= v <= n for v in lens) and len(set(lens)) == len(lens)
    assert {nsc.skipped_stages(PADDED_LOG_N, first, v) for v in lens if v} == set(range(first + 1))
    for k in range(1, first + 1):  # both sides of each threshold
        assert nsc.skipped_stages(PADDED_LOG_N, first, n >> k) == k and nsc.skipped_stages(PADDED_LOG_N, first, (n >> k) + 1) == k - 1
        assert (n >> k) in lens and (n >> k) + 1 in lens and max((n >> k) - 1, 0) in lens


@pytest.mark.parametrize("f", [br.TWEEDLEDEE_BASE, br.BLS12_377_BASE], ids=lambda f: f.name)
def test_padded_expectation_is_the_oracles_fft_with_precomputation(f):
    log_n = PADDED_LOG_N
    n = 1 << log_n
    opre = ol.FftPrecomputation(f.field_id, n)
    lens = sorted(set().union(*[nsc.padded_lengths(log_n, first) for first in PADDED_FIRST]))
    for src in (nsc.random_vector(f, log_n, salt=1), nsc.pattern_cycle(f, n)):
        for in_len in lens:
            x = np.ascontiguousarray(src[:in_len])
            exp = opre.fft_with_precomputation_power_of_2(nsc.padded(x, n))
            assert np.array_equal(exp, mont_arr(f, br.ntt(f, from_mont_arr(f, x) + [0] * (n - in_len)))), in_len
            if in_len == 0:
                assert not exp.any()
                continue
            got = opre.fft_with_precomputation(x)
            assert n % got.shape[0] == 0 and got.shape[0] >= in_len and (got.shape[0] == 1 or got.shape[0] < 2 * in_len)
            assert np.array_equal(got, exp[:: n // got.shape[0]]), in_len
            if in_len > n // 2:
                assert got.shape[0] == n
