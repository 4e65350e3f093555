"""GPU tests of the grand product Z of Plonk's permutation argument (plk_plonk_permutation_z[_dev], plonk_util.rs:234-262):
bit-exact parity with a Python restatement of the reference loop, edge words, zero denominators, honest copy cycles at full
size, host / device agreement, and the quotient path end to end on a satisfied circuit whose Z is not 1."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from plonky_amd import api
from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from tests.test_oracle_plonk import ZETA_MONT, mont, unmont

FIELDS = [br.TWEEDLEDEE_BASE, br.TWEEDLEDUM_BASE, br.BLS12_377_SCALAR, br.PALLAS_BASE, br.VESTA_BASE]


def z_restated(f, log_n, w, s, k, beta, gamma):
    """plonk_util.rs:234-262 on canonical ints (w[j][r], s[j][r]: the n-point sigma values), plus the status words of the
    device entry: zero denominators among rows 0..n-2, and whether the product over all n rows is 1."""
    p, n = f.p, 1 << log_n
    g = f.primitive_root_of_unity(log_n)
    z, x, zeros, wrap, closed = [1], 1, 0, 1, True
    for r in range(n):
        num = den = 1
        for j in range(6):
            num = num * (w[j][r] + beta * (k[j] * x) + gamma) % p
            den = den * (w[j][r] + beta * s[j][r] + gamma) % p
        if den == 0:
            zeros += r < n - 1
            closed = False
            den = 1
        wrap = wrap * num * pow(den, -1, p) % p
        if r < n - 1:
            z.append(z[-1] * num * pow(den, -1, p) % p)
        x = x * g % p
    return z, [zeros, int(closed and wrap == 1)]


def random_case(f, log_n, seed, stride):
    rng = random.Random(seed)
    n, p = 1 << log_n, f.p
    w = [[rng.randrange(p) for _ in range(n)] for _ in range(9)]
    s_full = [[rng.randrange(p) for _ in range(n * stride)] for _ in range(6)]
    k = [rng.randrange(p) for _ in range(6)]
    beta, gamma = rng.randrange(p), rng.randrange(p)
    return w, s_full, k, beta, gamma


def to_dev_args(f, w, s_full, k, beta, gamma):
    return (np.stack([mont(f, row) for row in w]), np.stack([mont(f, row) for row in s_full]), mont(f, k), mont(f, [beta])[0], mont(f, [gamma])[0])


def run_dev(f, log_n, wm, sm, km, bm, gm, stride, stream=None):
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    if stream is None:
        z, st = dev.permutation_polynomial_dev(f.field_id, log_n, dev.to_device(wm), dev.to_device(sm), km, bm, gm, sigma_stride=stride, status=True)
    else:
        with torch.cuda.stream(stream):
            z, st = dev.permutation_polynomial_dev(f.field_id, log_n, dev.to_device(wm), dev.to_device(sm), km, bm, gm, sigma_stride=stride, status=True)
        stream.synchronize()
    return dev.to_host(z), [int(v) for v in st.cpu().tolist()]


@pytest.mark.parametrize("stride", [8, 1])
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 6, 10, 13])
@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_z_matches_restatement(f, log_n, stride):
    w, s_full, k, beta, gamma = random_case(f, log_n, 0x2A + 97 * log_n + stride, stride)
    exp, exp_status = z_restated(f, log_n, w, [row[::stride] for row in s_full], k, beta, gamma)
    args = to_dev_args(f, w, s_full, k, beta, gamma)
    got = api.permutation_polynomial(f.field_id, 1 << log_n, *args, sigma_stride=stride)
    assert unmont(f, got) == exp
    if log_n == 0:
        assert exp == [1]
    got_d, status = run_dev(f, log_n, *args, stride)
    assert np.array_equal(got_d, got) and status == exp_status


def den_rows(f, log_n, w, s, beta, gamma):
    p = f.p
    return [np.prod([(w[j][r] + beta * s[j][r] + gamma) % p for j in range(6)], dtype=object) % p for r in range(1 << log_n)]


@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_z_edge_words(f):
    """Wires and sigma drawn from edge words (0, 1, p - 1, p - 2, ...) under the edge challenges beta = gamma = 0,
    beta = gamma = p - 1, beta = p - 1 / gamma = 0, beta = 1 / gamma = p - 1, with k_j = 1, k_j = p - 1 or random.  Every setting
    reaches the kernel twice: on the raw edge table (which has zero denominators for most settings: the status words must match
    the restatement, Z must match on the rows before the first zero, and the host entry must raise "No inverse"), and on the same
    table with every row r <= n - 2 whose den is zero redrawn from the edge words until it is not (full comparison)."""
    p, log_n = f.p, 6
    n = 1 << log_n
    rng = random.Random(0xED6E)
    edge = [0, 1, p - 1, p - 2, (p - 1) // 2, 1 << 250, p >> 1]
    settings = [([1] * 6, 0, 0), ([1] * 6, p - 1, p - 1), ([p - 1] * 6, 0, 5), ([rng.randrange(p) for _ in range(6)], p - 1, 0),
                ([p - 1] * 6, 1, p - 1), ([1] * 6, p - 1, 0)]
    raw_with_zeros = full_runs = 0
    for k, beta, gamma in settings:
        w = [[rng.choice(edge) for _ in range(n)] for _ in range(9)]
        s = [[rng.choice(edge) for _ in range(n)] for _ in range(6)]
        exp, exp_status = z_restated(f, log_n, w, s, k, beta, gamma)
        args = to_dev_args(f, w, s, k, beta, gamma)
        got, status = run_dev(f, log_n, *args, 1)
        assert status == exp_status, (k[0], beta, gamma)
        dens = den_rows(f, log_n, w, s, beta, gamma)
        first_zero = next((r for r in range(n - 1) if dens[r] == 0), None)
        if first_zero is None:
            assert unmont(f, got) == exp
        else:
            raw_with_zeros += 1
            assert status[0] > 0
            assert unmont(f, got)[: first_zero + 1] == exp[: first_zero + 1]  # Z[i] for i <= r reads rows < r only
            with pytest.raises(AssertionError, match="No inverse"):
                api.permutation_polynomial(f.field_id, n, *args, sigma_stride=1)
        # the same edge words without a zero denominator in rows 0..n-2
        for r in range(n - 1):
            tries = 0
            while dens[r] == 0:
                for j in range(6):
                    w[j][r], s[j][r] = rng.choice(edge), rng.choice(edge)
                dens[r] = den_rows(f, 0, [[w[j][r]] for j in range(6)], [[s[j][r]] for j in range(6)], beta, gamma)[0]
                tries += 1
                assert tries < 1000
        exp, exp_status = z_restated(f, log_n, w, s, k, beta, gamma)
        assert exp_status[0] == 0
        args = to_dev_args(f, w, s, k, beta, gamma)
        got, status = run_dev(f, log_n, *args, 1)
        assert unmont(f, got) == exp and status == exp_status, (k[0], beta, gamma)
        assert unmont(f, api.permutation_polynomial(f.field_id, n, *args, sigma_stride=1)) == exp
        full_runs += 1
    assert full_runs == len(settings) and raw_with_zeros >= 3, (full_runs, raw_with_zeros)
    # one row r = n - 2 with den = p - 1: factors 1, ..., 1, p - 1 (w = 0, beta = 1, gamma = 0, sigma = 1 / p - 1)
    w2 = [[rng.randrange(p) for _ in range(n)] for _ in range(9)]
    s2 = [[rng.randrange(p) for _ in range(n)] for _ in range(6)]
    for j in range(6):
        w2[j][n - 2], s2[j][n - 2] = 0, (p - 1 if j == 0 else 1)
    k = [rng.randrange(p) for _ in range(6)]
    exp, exp_status = z_restated(f, log_n, w2, s2, k, 1, 0)
    got, status = run_dev(f, log_n, *to_dev_args(f, w2, s2, k, 1, 0), 1)
    assert unmont(f, got) == exp and status == exp_status


def honest_copy_cycles(f, log_n, routed, k_m, key=None):
    """sigma (6, n, 4) for wire values `routed` (6, n, 4, Montgomery): the cells holding one value form one cycle, and
    sigma_j[r] = k_j' g^r' of the next cell (j', r') of that cycle.  The identity table k_j g^r comes from the device NTT of
    the polynomials k_j X (natural order: the evaluation at g^r is row r).  key: a label per cell that is equal exactly where the
    values are (np.unique of the values when not given)."""
    from plonky_amd import device as dev
    n = 1 << log_n
    coeffs = np.zeros((6, n, 4), dtype=np.uint64)
    coeffs[:, 1] = k_m
    ident = dev.to_host(dev.ntt_dev(f.field_id, dev.to_device(coeffs))).reshape(6 * n, 4)
    flat = routed.reshape(6 * n, 4)
    if key is None:
        key = np.unique(flat, axis=0, return_inverse=True)[1]
    key = np.asarray(key).reshape(-1)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    nxt = np.empty(6 * n, dtype=np.int64)
    last_of_group = np.append(ks[1:] != ks[:-1], True)
    first_idx = np.zeros(6 * n, dtype=np.int64)
    starts = np.flatnonzero(np.insert(ks[1:] != ks[:-1], 0, True))
    first_idx[starts] = starts
    first_idx = np.maximum.accumulate(first_idx)
    succ = np.arange(1, 6 * n + 1)
    succ[last_of_group] = first_idx[last_of_group]
    nxt[order] = order[succ]
    return ident[nxt].reshape(6, n, 4), ident.reshape(6, n, 4)


def pooled_wires(f, log_n, seed, pool_size=1 << 10):
    """(9, n, 4) wire values drawn from a pool of distinct values, and the pool index of every cell"""
    rng = np.random.default_rng(seed)
    r, vals = random.Random(seed), set()
    while len(vals) < pool_size:
        vals.add(r.randrange(1, f.p))
    pool = mont(f, sorted(vals))
    idx = rng.integers(0, pool_size, size=9 << log_n)
    return pool[idx].reshape(9, 1 << log_n, 4), idx.reshape(9, 1 << log_n)


def check_honest_z(f, log_n, w_host, sigma, z, k, beta, gamma, seed):
    p, n = f.p, 1 << log_n
    g = f.primitive_root_of_unity(log_n)
    z_i = lambda r: f.from_mont(br.limbs_to_int(z[r]))

    def nd(r):
        x, num, den = pow(g, r, p), 1, 1
        for j in range(6):
            wv, sv = f.from_mont(br.limbs_to_int(w_host[j, r])), f.from_mont(br.limbs_to_int(sigma[j, r]))
            num = num * (wv + beta * k[j] * x + gamma) % p
            den = den * (wv + beta * sv + gamma) % p
        return num, den

    assert z_i(0) == 1
    rng = random.Random(seed)
    for i in [1, n - 1] + [rng.randrange(1, n) for _ in range(254)]:
        num, den = nd(i - 1)
        assert z_i(i) * den % p == z_i(i - 1) * num % p, i
    num, den = nd(n - 1)
    assert z_i(n - 1) * num % p == den


@pytest.mark.parametrize("log_n", [16, 20, 22])
def test_honest_permutation_closes(log_n):
    """A satisfied copy-constraint table closes the cycle.  At 2^22 rows there are 2048 tiles of 2048 rows: every lane of the tile scan
    (k_perm_tiles, 1024 lanes) carries two of them."""
    from plonky_amd import device as dev
    dev.init(0)
    f, n = br.TWEEDLEDUM_BASE, 1 << log_n
    rng = random.Random(0x5161 + log_n)
    k = [rng.randrange(f.p) for _ in range(6)]
    beta, gamma = rng.randrange(f.p), rng.randrange(f.p)
    km, bm, gm = mont(f, k), mont(f, [beta])[0], mont(f, [gamma])[0]
    w, idx = pooled_wires(f, log_n, 0xC0DE + log_n)
    sigma, _ = honest_copy_cycles(f, log_n, w[:6], km, key=idx[:6])
    dw, ds = dev.to_device(w), dev.to_device(sigma)
    z, st = dev.permutation_polynomial_dev(f.field_id, log_n, dw, ds, km, bm, gm, sigma_stride=1, status=True)
    assert st.cpu().tolist() == [0, 1]
    check_honest_z(f, log_n, w, sigma, dev.to_host(z), k, beta, gamma, log_n)
    # two sigma entries of different values swapped: the cycles no longer match the wire values
    bad = sigma.copy()
    a, b = (0, 5), (3, n - 7)
    assert idx[a] != idx[b]
    bad[a], bad[b] = sigma[b].copy(), sigma[a].copy()
    _, st = dev.permutation_polynomial_dev(f.field_id, log_n, dw, dev.to_device(bad), km, bm, gm, sigma_stride=1, status=True)
    assert st.cpu().tolist()[1] == 0


LARGE_FIELDS = [br.TWEEDLEDEE_BASE, br.BLS12_377_SCALAR, br.PALLAS_BASE, br.VESTA_BASE]


@pytest.mark.parametrize("log_n,stride", [(21, 8), (22, 1)], ids=["2p21-stride8", "2p22-stride1"])
@pytest.mark.parametrize("f", LARGE_FIELDS, ids=lambda f: f.name)
def test_z_random_large_n(f, log_n, stride):
    """Random wires and sigma drawn on the device (every element independent).  2^21 rows: 1024 tiles, exactly one per lane of the
    tile scan, sigma read with stride 8 from an 8n table; 2^22 rows: two tiles per scan lane.  The recurrence
    z[i] den[i-1] == z[i-1] num[i-1] is checked with big integers at every tile boundary i = 2048 k (the steps within a scan lane and
    between lanes) and at 1024 seeded random rows; z[0] = 1, no zero denominator, and status[1] is what the returned Z says."""
    import torch
    from plonky_amd import device as dev
    from tests.test_gpu_plonk_fullsize import clear_device_caches, device_words
    dev.init(0)
    p, n = f.p, 1 << log_n
    seed = 0x2B16 + 16 * log_n + f.field_id
    rng = random.Random(seed)
    km = ol.rand_field(f.field_id, seed, 8)
    km, bm, gm = km[:6], km[6], km[7]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    tile = 2048
    boundaries = list(range(tile, n, tile))
    assert len(boundaries) == n // tile - 1
    checked = sorted(set(boundaries) | set(rng.sample(range(1, n), 1024)) | {n - 1})
    rows = sorted(set(checked) | {i - 1 for i in checked} | {0})
    try:
        w = device_words(f, (6, n), gen)
        s = device_words(f, (6, n * stride), gen)
        z, st = dev.permutation_polynomial_dev(f.field_id, log_n, w, s, km, bm, gm, sigma_stride=stride, status=True)
        r_t = torch.tensor(rows, dtype=torch.int64, device="cuda")
        wh = dev.to_host(w[:, r_t])
        sh = dev.to_host(s.view(6, n, stride, 4)[:, r_t, 0])
        zh = dev.to_host(z[r_t])
        status = [int(v) for v in st.cpu().tolist()]
    finally:
        w = s = z = None
        clear_device_caches()
    at = {r: c for c, r in enumerate(rows)}
    canon = lambda v: f.from_mont(br.limbs_to_int(v))
    k = [canon(km[j]) for j in range(6)]
    beta, gamma = canon(bm), canon(gm)
    g = f.primitive_root_of_unity(log_n)
    assert all(br.limbs_to_int(v) < p for v in zh), "Z words are not canonical"
    z_i = lambda r: canon(zh[at[r]])

    def nd(r):
        x, num, den = pow(g, r, p), 1, 1
        for j in range(6):
            wv, sv = canon(wh[j, at[r]]), canon(sh[j, at[r]])
            num = num * (wv + beta * k[j] * x + gamma) % p
            den = den * (wv + beta * sv + gamma) % p
        return num, den

    assert br.limbs_to_int(zh[at[0]]) == f.to_mont(1)
    assert status[0] == 0
    bad = []
    for i in checked:
        num, den = nd(i - 1)
        if z_i(i) * den % p != z_i(i - 1) * num % p:
            bad.append(i)
    assert not bad, "%d of %d checked rows break the recurrence, first %s" % (len(bad), len(checked), bad[:8])
    num, den = nd(n - 1)
    assert status[1] == int(z_i(n - 1) * num % p == den)


@pytest.mark.parametrize("where", ["middle", "last"])
def test_zero_denominator(where):
    f, log_n = br.TWEEDLEDEE_BASE, 8
    n, p = 1 << log_n, f.p
    w, s, k, beta, _ = random_case(f, log_n, 0x2E80, 1)
    r = n // 2 if where == "middle" else n - 1
    gamma = (-(w[0][r] + beta * s[0][r])) % p  # factor j = 0 of den_r vanishes
    exp, exp_status = z_restated(f, log_n, w, s, k, beta, gamma)
    args = to_dev_args(f, w, s, k, beta, gamma)
    _, status = run_dev(f, log_n, *args, 1)
    if where == "middle":
        assert exp_status[0] == 1 and status[0] == 1 and status[1] == 0
        with pytest.raises(AssertionError, match="No inverse"):
            api.permutation_polynomial(f.field_id, n, *args, sigma_stride=1)
    else:
        assert status == [0, 0] == exp_status
        assert unmont(f, api.permutation_polynomial(f.field_id, n, *args, sigma_stride=1)) == exp


def test_host_and_device_agree_strides_and_streams():
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    f, log_n = br.BLS12_377_SCALAR, 11
    n = 1 << log_n
    w, s8, k, beta, gamma = random_case(f, log_n, 0x57AE, 8)
    args = to_dev_args(f, w, s8, k, beta, gamma)
    copies = [a.copy() for a in args]
    host = api.permutation_polynomial(f.field_id, n, *args, sigma_stride=8)
    for a, c in zip(args, copies):
        assert np.array_equal(a, c), "inputs modified"
    side = torch.cuda.Stream()
    got, status = run_dev(f, log_n, *args, 8, stream=side)
    assert np.array_equal(got, host)
    ws, ss = dev.to_device(args[0]), dev.to_device(args[1])
    dev.permutation_polynomial_dev(f.field_id, log_n, ws, ss, *args[2:], sigma_stride=8)
    torch.cuda.synchronize()
    assert np.array_equal(dev.to_host(ws), args[0]) and np.array_equal(dev.to_host(ss), args[1]), "device inputs modified"
    extract = np.ascontiguousarray(args[1].reshape(6, 8 * n, 4)[:, ::8])
    assert np.array_equal(api.permutation_polynomial(f.field_id, n, args[0], extract, *args[2:], sigma_stride=1), host)
    assert np.array_equal(api.permutation_polynomial(f.field_id, n, args[0][:6], extract, *args[2:], sigma_stride=1), host)


def test_quotient_end_to_end_with_real_copy_constraints():
    """ArithmeticGate rows (w3 = c0 w0 w1 + c1 w2) whose other routed wires repeat values, one copy cycle per value.  Device
    chain: Z (stride 8 on s_sigma_values_8n) -> iNTT -> LDE -> vanishing points -> iNTT -> divide_by_z_h: exact, deg q < 7n;
    with Z = 1 instead the division leaves a remainder."""
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    f, log_n = br.TWEEDLEDUM_BASE, 12
    F, n = f.field_id, 1 << log_n
    rng = random.Random(0xE2E)
    w, _ = pooled_wires(f, log_n, 0xE2E, pool_size=200)
    c0, c1 = (mont(f, [rng.randrange(f.p) for _ in range(n)]) for _ in range(2))
    w[3] = api.field_op(F, "add", api.field_op(F, "mul", api.field_op(F, "mul", c0, w[0]), w[1]), api.field_op(F, "mul", c1, w[2]))
    one, zero = mont(f, [1])[0], mont(f, [0])[0]
    consts = np.stack([np.tile(one, (n, 1)), np.tile(zero, (n, 1)), np.tile(zero, (n, 1)), np.tile(one, (n, 1)), c0, c1])
    k = [rng.randrange(f.p) for _ in range(6)]
    km = mont(f, k)
    alpha, beta, gamma = (mont(f, [rng.randrange(f.p)])[0] for _ in range(3))
    sigma_n, _ = honest_copy_cycles(f, log_n, w[:6], km)
    cols = dev.to_device(np.concatenate([consts, w, sigma_n]))                           # (21, n, 4)
    lde = dev.ntt_padded_dev(F, dev.ntt_dev(F, cols, inverse=True), log_n + 3)
    consts_8n, wires_8n, sigma_8n = lde[:6].contiguous(), lde[6:15].contiguous(), lde[15:].contiguous()
    wires_n = dev.to_device(w)
    z, st = dev.permutation_polynomial_dev(F, log_n, wires_n, sigma_8n, km, beta, gamma, sigma_stride=8, status=True)
    assert st.cpu().tolist() == [0, 1]
    zh = dev.to_host(z)
    assert len({tuple(r) for r in zh[:64]}) > 32, "Z is not constant"

    def quotient(zvals):
        z_8n = dev.ntt_padded_dev(F, dev.ntt_dev(F, zvals, inverse=True), log_n + 3)
        pts = dev.vanishing_points_dev(F, log_n, consts_8n, wires_8n, sigma_8n, z_8n, km, alpha, beta, gamma, np.array(ZETA_MONT, dtype=np.uint64), zero)
        vanishing = dev.ntt_dev(F, pts, inverse=True)
        t = dev.divide_by_z_h_dev(F, vanishing, n, out=torch.empty((8 * n, 4), dtype=torch.int64, device="cuda"))
        torch.cuda.synchronize()
        v, q = dev.to_host(vanishing), np.zeros((8 * n, 4), dtype=np.uint64)
        th = dev.to_host(t)
        q[: th.shape[0]] = th
        zpad = np.zeros((n, 4), dtype=np.uint64)
        back = api.field_op(F, "sub", np.concatenate([zpad, q[: 7 * n]]), np.concatenate([q[: 7 * n], zpad]))
        return v, q, back

    v, q, back = quotient(z)
    assert v.any() and not q[7 * n:].any() and np.array_equal(back, v)
    v1, _, back1 = quotient(dev.to_device(np.tile(one, (n, 1))))
    assert not np.array_equal(back1, v1), "the quotient path does not see Z"
