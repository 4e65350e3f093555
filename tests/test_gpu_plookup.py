"""GPU tests of the Plookup prover's two device loops (plk_plookup_grand_product[_dev], plk_plookup_vanishing_points[_dev]): bit-exact
parity with the big-integer restatements of tests/plookup_ref.py on the five fields, edge words and zero denominators, honest
witnesses, host / device / stream agreement, the prover's chain end to end over device entries only, and the refusals.

Sizes of the grand product: the row kernel's tile is LKP_ROWS x LKP_LANES = 4 x 128 = 512 rows (plookup.hip) and the tile scan
(k_perm_tiles) gives one tile to each of its 1024 lanes, 64 lanes a wave.  So besides the small sizes 1, 2, 3, 4, 6: log_size 9 is one tile
exactly, 10 two tiles (the tile scan and the fix-up do work), 16 is 128 tiles - more than the 64 lanes of one wave of the tile scan, so
its cross-wave step runs."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from plonky_amd import api
from plonky_amd import lib as plk
from tests import checked_child
from tests import plookup_ref as pr
from tests.test_oracle_plonk import mont, unmont

FIELDS = [br.TWEEDLEDEE_BASE, br.TWEEDLEDUM_BASE, br.BLS12_377_SCALAR, br.PALLAS_BASE, br.VESTA_BASE]
ONE_TILE, TWO_TILES, MANY_TILES = 9, 10, 16


def one(f, v):
    return mont(f, [v])[0]


def product_args(f, fv, t, s, beta, gamma):
    """f_padded, t, s as limb arrays, and the two challenges"""
    return mont(f, fv + [0]), mont(f, t), mont(f, s), one(f, beta), one(f, gamma)


def run_product_dev(f, log_size, fm, tm, sm, bm, gm, stream=None):
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    if stream is None:
        z, st = dev.plookup_grand_polynomial_dev(f.field_id, log_size, dev.to_device(fm), dev.to_device(tm), dev.to_device(sm), bm, gm, status=True)
    else:
        with torch.cuda.stream(stream):
            z, st = dev.plookup_grand_polynomial_dev(f.field_id, log_size, dev.to_device(fm), dev.to_device(tm), dev.to_device(sm), bm, gm, status=True)
        stream.synchronize()
    return dev.to_host(z), [int(v) for v in st.cpu().tolist()]


def random_product_case(f, log_size, seed):
    rng = random.Random(seed)
    n, p = (1 << log_size) - 1, f.p
    return ([rng.randrange(p) for _ in range(n)], [rng.randrange(p) for _ in range(n + 1)], [rng.randrange(p) for _ in range(2 * n + 1)],
            rng.randrange(p), rng.randrange(p))


@pytest.mark.parametrize("log_size", [1, 2, 3, 4, 6, ONE_TILE, TWO_TILES, MANY_TILES])
@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_grand_product_matches_restatement(f, log_size):
    import torch
    case = random_product_case(f, log_size, 0x9100 + 31 * log_size + f.field_id)
    exp, exp_status = pr.grand_polynomial(f, *case)
    assert exp_status[0] == 0
    args = product_args(f, *case)
    copies = [a.copy() for a in args]
    got, closes = api.plookup_grand_polynomial(f.field_id, *args, return_closes=True)
    assert all(np.array_equal(a, c) for a, c in zip(args, copies)), "inputs modified"
    assert unmont(f, got) == exp and closes == bool(exp_status[1])
    got_d, status = run_product_dev(f, log_size, *args)
    assert np.array_equal(got_d, got) and status == exp_status
    got_s, status_s = run_product_dev(f, log_size, *args, stream=torch.cuda.Stream())
    assert np.array_equal(got_s, got) and status_s == exp_status


def den_rows(f, t, s, beta, gamma):
    p, n = f.p, len(t) - 1
    gb1 = gamma * (beta + 1) % p
    return [(gb1 + s[j] + beta * s[j + 1]) * (gb1 + s[n + j] + beta * s[n + j + 1]) % p for j in range(n)]


@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_grand_product_edge_words(f):
    """f, t, s drawn from {0, 1, p - 1, p - 2, (p - 1) / 2} under every beta, gamma in {0, 1, p - 1} (beta = p - 1 makes beta + 1 = 0:
    every numerator vanishes).  The status words must match the restatement; the output must match it on the rows before the first
    zero denominator (all rows when there is none), and the host form raises "No inverse" exactly when rows 0..n-2 hold one."""
    p, log_size = f.p, 6
    n = (1 << log_size) - 1
    rng = random.Random(0xED6F + f.field_id)
    edge = [0, 1, p - 1, p - 2, (p - 1) // 2]
    with_zero = without = 0
    for beta in (0, 1, p - 1):
        for gamma in (0, 1, p - 1):
            fv, t, s = [rng.choice(edge) for _ in range(n)], [rng.choice(edge) for _ in range(n + 1)], [rng.choice(edge) for _ in range(2 * n + 1)]
            exp, exp_status = pr.grand_polynomial(f, fv, t, s, beta, gamma)
            args = product_args(f, fv, t, s, beta, gamma)
            got, status = run_product_dev(f, log_size, *args)
            assert status == exp_status, (beta, gamma)
            dens = den_rows(f, t, s, beta, gamma)
            first_zero = next((j for j in range(n - 1) if dens[j] == 0), None)
            if first_zero is None:
                without += 1
                assert unmont(f, got) == exp, (beta, gamma)
                assert unmont(f, api.plookup_grand_polynomial(f.field_id, *args)) == exp
            else:
                with_zero += 1
                assert status[0] > 0 and status[1] == 0
                assert unmont(f, got)[: first_zero + 1] == exp[: first_zero + 1]  # values[i] for i <= j reads rows < j only
                with pytest.raises(AssertionError, match="No inverse"):
                    api.plookup_grand_polynomial(f.field_id, *args)
    assert with_zero >= 1 and with_zero + without == 9
    # a zero denominator in the LAST row only: no panic, the output is complete, the argument does not close
    fv, t, s, beta, _ = random_product_case(f, log_size, 0x1A57)
    gamma_beta1 = (-(s[n - 1] + beta * s[n])) % p
    gamma = gamma_beta1 * pow(beta + 1, -1, p) % p
    exp, exp_status = pr.grand_polynomial(f, fv, t, s, beta, gamma)
    assert exp_status == [0, 0] and den_rows(f, t, s, beta, gamma)[n - 1] == 0
    args = product_args(f, fv, t, s, beta, gamma)
    got, status = run_product_dev(f, log_size, *args)
    assert unmont(f, got) == exp and status == exp_status
    assert unmont(f, api.plookup_grand_polynomial(f.field_id, *args)) == exp


def honest_witness(f, log_size, seed):
    """t random and distinct, f drawn from t with repeats, s from the host helper (limb arrays; f has n rows)"""
    rng = random.Random(seed)
    n = (1 << log_size) - 1
    tv = set()
    while len(tv) < n + 1:
        tv.add(rng.randrange(f.p))
    t = list(tv)
    rng.shuffle(t)
    fv = [rng.choice(t) for _ in range(n)]
    tm, fm = mont(f, t), mont(f, fv)
    return fv, t, fm, tm, api.plookup_sorted_multiset(fm, tm)


@pytest.mark.parametrize("log_size", [6, 12])
def test_honest_witness_closes(log_size):
    f = br.TWEEDLEDUM_BASE
    rng = random.Random(0x40E5 + log_size)
    fv, t, fm, tm, sm = honest_witness(f, log_size, 0x5EED + log_size)
    beta, gamma = rng.randrange(f.p), rng.randrange(f.p)
    fpad = np.concatenate([fm, np.zeros((1, 4), dtype=np.uint64)])
    z, status = run_product_dev(f, log_size, fpad, tm, sm, one(f, beta), one(f, gamma))
    assert status == [0, 1]
    zi = unmont(f, z)
    assert zi[0] == 1 and zi[-1] == 1 and len(set(zi)) > len(zi) // 2, "Z is not constant"
    # one f value replaced by an element outside t (s keeps the honest multiset's size: the outsider sorts to the front)
    outsider = next(v for v in range(2, 1000) if v not in set(t))
    bad = fpad.copy()
    bad[len(fv) // 3] = one(f, outsider)
    _, status = run_product_dev(f, log_size, bad, tm, sm, one(f, beta), one(f, gamma))
    assert status[1] == 0


def run_points_dev(f, log_size, rows, am, bm, gm):
    from plonky_amd import device as dev
    dev.init(0)
    return dev.to_host(dev.plookup_vanishing_values_dev(f.field_id, log_size, dev.to_device(rows), am, bm, gm))


@pytest.mark.parametrize("log_size", [1, 2, 3, 6, 10])
@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_vanishing_points_match_restatement(f, log_size):
    """random rows: no term vanishes except through eval_l_i's zeros; all 4N points are compared"""
    rng = random.Random(0x7A00 + 13 * log_size + f.field_id)
    n4, p = 4 << log_size, f.p
    rows = [[rng.randrange(p) for _ in range(n4)] for _ in range(5)]
    alpha, beta, gamma = (rng.randrange(p) for _ in range(3))
    exp = pr.vanishing_values(f, log_size, *rows, alpha, beta, gamma)
    rm = np.stack([mont(f, r) for r in rows])
    sc = [one(f, v) for v in (alpha, beta, gamma)]
    got = api.plookup_vanishing_values(f.field_id, rm, *sc)
    assert unmont(f, got) == exp
    assert np.array_equal(run_points_dev(f, log_size, rm, *sc), got)
    # at i = 0 (mod 4) both Lagrange factors are 0 and only the shift term is left; its factor x - w^n removes it at i = 4 n alone
    assert [v != 0 for v in exp[::4]] == [True] * ((1 << log_size) - 1) + [False]


def lde_rows(f, log_size, z, fpad, tm, sm):
    """device: the five polynomials (coefficients) and their values on the 4N domain, rows z, f, t, h1, h2"""
    from plonky_amd import device as dev
    n = (1 << log_size) - 1
    cols = dev.to_device(np.stack([z, fpad, tm, sm[: n + 1], sm[n:]]))
    coeffs = dev.ntt_dev(f.field_id, cols, inverse=True)
    return coeffs, dev.ntt_padded_dev(f.field_id, coeffs, log_size + 2)


def test_vanishing_points_on_honest_ldes():
    from plonky_amd import device as dev
    dev.init(0)
    f, log_size = br.PALLAS_BASE, 6
    rng = random.Random(0x10DE)
    fv, t, fm, tm, sm = honest_witness(f, log_size, 0xBEE)
    alpha, beta, gamma = (rng.randrange(f.p) for _ in range(3))
    fpad = np.concatenate([fm, np.zeros((1, 4), dtype=np.uint64)])
    z, status = run_product_dev(f, log_size, fpad, tm, sm, one(f, beta), one(f, gamma))
    assert status == [0, 1]
    _, lde = lde_rows(f, log_size, z, fpad, tm, sm)
    sc = [one(f, v) for v in (alpha, beta, gamma)]
    got = unmont(f, dev.to_host(dev.plookup_vanishing_values_dev(f.field_id, log_size, lde, *sc)))
    rows = [unmont(f, r) for r in dev.to_host(lde)]
    assert got == pr.vanishing_values(f, log_size, *rows, alpha, beta, gamma)
    assert not any(got[::4]) and any(got), "the vanishing polynomial vanishes on H, and only there"


def horner(p, coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def test_prover_chain_end_to_end():
    """prove (plookup.rs:16-88) up to the quotient on Tweedledee's scalar field, N = 2^10, device entries only: s on the host, four
    inverse transforms, the grand product, its inverse transform, five padded transforms to 4N, the vanishing points, the inverse
    transform, divide_by_z_h(N).  The quotient has at most 2 n + 1 coefficients (plookup.rs:86) and, at two random points x,
    quotient(x) (x^N - 1) is the vanishing polynomial evaluated with integers from the five polynomials at x and x w."""
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    f, log_size = br.TWEEDLEDUM_BASE, 10
    F, p, size = f.field_id, f.p, 1 << log_size
    n = size - 1
    rng = random.Random(0xE2E10)
    fv, t, fm, tm, sm = honest_witness(f, log_size, 0xFACE)
    alpha, beta, gamma = (rng.randrange(p) for _ in range(3))
    am, bm, gm = (one(f, v) for v in (alpha, beta, gamma))
    fpad = dev.to_device(np.concatenate([fm, np.zeros((1, 4), dtype=np.uint64)]))
    sd = dev.to_device(sm)
    cols = torch.stack([fpad, dev.to_device(tm), sd[:size], sd[n:]]).contiguous()
    polys = dev.ntt_dev(F, cols, inverse=True)                                        # f, t, h1, h2
    z, st = dev.plookup_grand_polynomial_dev(F, log_size, fpad, cols[1], sd, bm, gm, status=True)
    assert st.cpu().tolist() == [0, 1]
    z_poly = dev.ntt_dev(F, z, inverse=True)
    five = torch.cat([z_poly[None], polys]).contiguous()                               # z, f, t, h1, h2
    lde = dev.ntt_padded_dev(F, five, log_size + 2)
    pts = dev.plookup_vanishing_values_dev(F, log_size, lde, am, bm, gm)
    vanishing = dev.ntt_dev(F, pts, inverse=True)
    quotient = dev.divide_by_z_h_dev(F, vanishing, size)
    torch.cuda.synchronize()
    q = unmont(f, dev.to_host(quotient))
    while q and q[-1] == 0:
        q.pop()
    assert 0 < len(q) <= 2 * n + 1
    zc, fc, tc, h1c, h2c = (unmont(f, c) for c in dev.to_host(five))
    w = f.primitive_root_of_unity(log_size)
    last_root = pow(w, n, p)
    beta1 = (beta + 1) % p
    gb1 = gamma * beta1 % p
    for _ in range(2):
        x = rng.randrange(2, p)
        xw = x * w % p
        zh = (pow(x, size, p) - 1) % p
        l0 = zh * pow(size * (x - 1), -1, p) % p
        ln = last_root * zh * pow(size * (x - last_root), -1, p) % p
        zx, znx = horner(p, zc, x), horner(p, zc, xw)
        shift = (x - last_root) * (zx * beta1 * (gamma + horner(p, fc, x)) * (gb1 + horner(p, tc, x) + beta * horner(p, tc, xw))
                                   - znx * (gb1 + horner(p, h1c, x) + beta * horner(p, h1c, xw)) * (gb1 + horner(p, h2c, x) + beta * horner(p, h2c, xw))) % p
        terms = [l0 * (zx - 1) % p, shift, ln * (horner(p, h1c, x) - horner(p, h2c, xw)) % p, ln * (zx - 1) % p]
        exp = sum(term * pow(alpha, k, p) for k, term in enumerate(terms)) % p
        assert horner(p, q, x) * zh % p == exp


BAD_FIELDS = (-1, 6, 1000)
NOT_SCALAR = "field %d is not a circuit scalar field"
P, S = "P", "S"
CALLS = {  # entry -> arguments after (log_size, field)
    "plk_plookup_grand_product_dev": (P, P, P, P, P, P, P, S),
    "plk_plookup_grand_product": (P, P, P, P, P, P, P),
    "plk_plookup_vanishing_points_dev": (P, P, P, P, P, S),
    "plk_plookup_vanishing_points": (P, P, P, P, P),
}


@pytest.fixture(scope="module")
def pinned():
    """64 KiB of pinned memory that host and device can both address: a call that did launch would do no harm"""
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    return torch.ones(8192, dtype=torch.int64).pin_memory()


def call(L, pinned, name, log_size, field):
    args = [pinned.data_ptr() if a == P else None for a in CALLS[name]]
    rc = getattr(L, name)(log_size, field, *args)
    return rc, L.plk_last_error().decode("utf-8", "replace")


@pytest.mark.parametrize("name", sorted(CALLS))
def test_unknown_field_is_refused(pinned, name):
    L = plk.load()
    for ident in BAD_FIELDS:
        rc, err = call(L, pinned, name, 2, ident)
        assert rc == plk.PLK_ERR_INVALID_ARG and err.startswith(NOT_SCALAR % ident), (name, ident, rc, err)
    rc, err = call(L, pinned, name, 2, 3)  # Bls12377Base: six limbs
    assert rc == plk.PLK_ERR_INVALID_ARG and err.startswith(NOT_SCALAR % 3), (name, rc, err)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_sizes_out_of_range_are_refused(pinned, name):
    L = plk.load()
    rc, err = call(L, pinned, name, 29, 0)
    assert rc == plk.PLK_ERR_TWO_ADICITY and "too large" in err, (name, rc, err)
    if "grand_product" in name:
        rc, err = call(L, pinned, name, 0, 0)
        assert rc == plk.PLK_ERR_INVALID_ARG and err.startswith("log_size 0"), (name, rc, err)


def run_small_set():
    """a reduced set for the checked build: both kernels, two fields, one and two tiles"""
    compared = 0
    for f in (br.TWEEDLEDEE_BASE, br.BLS12_377_SCALAR):
        for log_size in (3, TWO_TILES):
            case = random_product_case(f, log_size, 0xC4EC + log_size)
            exp, exp_status = pr.grand_polynomial(f, *case)
            got, status = run_product_dev(f, log_size, *product_args(f, *case))
            assert unmont(f, got) == exp and status == exp_status
            compared += 1
        rng = random.Random(0xC4ED)
        rows = [[rng.randrange(f.p) for _ in range(4 << 4)] for _ in range(5)]
        sc = [rng.randrange(f.p) for _ in range(3)]
        got = run_points_dev(f, 4, np.stack([mont(f, r) for r in rows]), *[one(f, v) for v in sc])
        assert unmont(f, got) == pr.vanishing_values(f, 4, *rows, *sc)
        compared += 1
    return compared


CHECKED_BODY = '''
from tests.test_gpu_plookup import run_small_set
print("CHECKED compared", run_small_set())
'''


def test_checked_build_runs_the_small_set():
    assert "CHECKED compared 6" in checked_child.run_checked(CHECKED_BODY)
