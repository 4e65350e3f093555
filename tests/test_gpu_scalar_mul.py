"""GPU: plk_curve_scalar_mul, plk_halo_n and plk_halo_n_mul against Python integers (oracle.bigint_ref, tests/halo_endo_ref.py), and the
inner-product argument's output checked by what it is for: the prover's L_j, R_j, final a, b, G and a Schnorr proof pass api.verify_ipa,
tampered values fail it.  Sizes are the smallest at which the kernels can go wrong (one wave per workgroup: 63 / 64 / 65, several
workgroups: 257, 1000), not the workload's."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from tests import checked_child
from tests import halo_endo_ref as he
from tests import scalar_mul_cases as sc
from tests.util import limbs_to_int

ALL_CURVES = (0, 1, 2, 3, 4)


def _dev():
    pytest.importorskip("torch")
    from plonky_amd import device as dev
    dev.init(0)
    return dev


def _mont(f, values):
    return np.array([f.mont_limbs(v) for v in values], dtype=np.uint64).reshape(-1, f.n_limbs)


def _ints(f, arr):
    return [f.from_mont(limbs_to_int(row)) for row in np.asarray(arr).reshape(-1, f.n_limbs)]


def _pt(curve, P):
    return sc.point_limbs(curve, P)[0]


def _to_point(curve, xy, zero):
    c = br.CURVES[curve]
    return None if int(zero) else (c.base.from_mont(limbs_to_int(xy[0])), c.base.from_mont(limbs_to_int(xy[1])))


# ---- shapes and aliasing ----
def _cyclic_pairs(curve, count):
    """`count` elements dealt from 24 distinct (scalar, point) pairs, so that the lanes of a wave carry different scalars and points
    while the expectation stays 24 big-integer multiplications"""
    base = sc.pairs(curve)
    pool = [base[(11 * k) % len(base)] for k in range(24)]
    return [pool[(7 * i) % 24] for i in range(count)]


@pytest.mark.parametrize("curve", (0, 2))
@pytest.mark.parametrize("count", (1, 3, 63, 64, 65, 257, 1000))
def test_scalar_mul_shapes(curve, count):
    dev = _dev()
    import torch
    from plonky_amd import api
    prs = _cyclic_pairs(curve, count)
    s, p, z = sc.pack(curve, prs)
    out, oz = api.curve_scalar_mul(curve, s, p, z)
    sc.check(curve, prs, out, oz)
    ds, dp, dz = dev.to_device(s), dev.to_device(p), torch.from_numpy(z).cuda()
    dout, doz = dev.scalar_mul_dev(curve, ds, dp, dz)
    dout2, doz2 = dev.scalar_mul_dev(curve, ds, dp, dz)
    torch.cuda.synchronize()
    assert np.array_equal(dev.to_host(dout), out) and np.array_equal(doz.cpu().numpy(), oz)       # host-pointer and _dev form: the same bytes
    assert torch.equal(dout, dout2) and torch.equal(doz, doz2)                                     # two runs are bit-identical
    dev.scalar_mul_dev(curve, ds, dp, dz, out=dp, out_zero=dz)                                     # in place
    torch.cuda.synchronize()
    assert np.array_equal(dev.to_host(dp), out) and np.array_equal(dz.cpu().numpy(), oz)


@pytest.mark.parametrize("curve", (0, 2))
def test_scalar_mul_broadcast(curve):
    dev = _dev()
    from plonky_amd import api
    prs = _cyclic_pairs(curve, 70)
    s, p, z = sc.pack(curve, prs)
    k0, P0 = prs[1]
    out, oz = api.curve_scalar_mul(curve, s[1], p, z)                     # 1 scalar x count points
    sc.check(curve, [(k0, P) for _, P in prs], out, oz)
    out, oz = api.curve_scalar_mul(curve, s, p[1], z[1:2])                # count scalars x 1 point
    sc.check(curve, [(k, P0) for k, _ in prs], out, oz)
    out, oz = api.curve_scalar_mul(curve, s[1], p[1])                     # 1 x 1
    sc.check(curve, [(k0, P0)], out, oz)
    if curve == 0:
        bits = [k & ((1 << 128) - 1) for k, _ in prs]
        exp = sc.expect(curve, [he.halo_n_mul(curve, he.bits_of(b, 128), P0) for b in bits[:8]])
        out, oz = api.halo_n_mul(curve, s[:8], p[1], z[1:2])              # the same shapes through halo_n_mul
        assert np.array_equal(out, exp[0]) and np.array_equal(oz, exp[1])
        exp = sc.expect(curve, [he.halo_n_mul(curve, he.bits_of(bits[1], 128), P) if P else None for _, P in prs[:8]])
        out, oz = api.halo_n_mul(curve, s[1], p[:8], z[:8])
        assert np.array_equal(out, exp[0]) and np.array_equal(oz, exp[1])


# ---- scalar_mul against big integers ----
def _bls_extra_points():
    """the 2-torsion point (-1, 0) and a point of the full group outside the r-subgroup (hash_to_curve clears no cofactor)"""
    from plonky_amd import api
    c = br.BLS12_377
    torsion = (c.base.p - 1, 0)
    assert br.ec_on_curve(c, torsion) and br.ec_add(c, torsion, torsion) is None
    outside = None
    for seed in range(8):
        xy = np.asarray(api.blake_hash_usize_to_curve(2, seed)).reshape(-1, 2, c.base.n_limbs)[0]
        P = _to_point(2, xy, 0)
        assert br.ec_on_curve(c, P)
        if br.ec_mul(c, c.scalar.p, P) is not None:
            outside = P
            break
    assert outside is not None, "no hashed point outside the r-subgroup among 8 seeds"
    return torsion, outside


def _all_pairs(curve):
    """the edge and seeded scalars over the points, and 2^k, 2^k - 1 on G for every k"""
    if curve != 2:
        return sc.pairs(curve) + sc.power_pairs(curve)
    torsion, outside = _bls_extra_points()
    r = br.BLS12_377.scalar.p
    prs = sc.pairs(curve, extra_points=(outside,))
    prs += [(k, torsion) for k in (0, 1, 2, 3, 4, r - 1, r - 2)]
    prs += [(k, outside) for k in (0, 1, 2, r - 1, r - 2, (r + 1) // 2)]   # [r - s] P != -[s] P out here: what the s -> r - s shortcut would break
    return prs + sc.power_pairs(curve)


@pytest.mark.parametrize("curve", ALL_CURVES)
def test_scalar_mul_matches_big_integers(curve):
    _dev()
    from plonky_amd import api
    prs = _all_pairs(curve)
    if curve in he.ENDO_CURVES:
        # the scalars chosen with the restated split are among the cases: (K, 0) at the largest such K, and halves of 129 bits
        chosen, longest = sc.glv_edge_scalars(curve)
        assert sc.glv_split(curve, chosen[0])[1] == 0 and chosen[0].bit_length() >= 127 and longest >= 129
        assert all((k, sc.base_points(curve)[0]) in prs for k in chosen)
    s, p, z = sc.pack(curve, prs)
    out, oz = api.curve_scalar_mul(curve, s, p, z)
    sc.check(curve, prs, out, oz)


CHECKED_BODY = '''
from plonky_amd import api, device as dev
from tests import scalar_mul_cases as sc
from tests.test_gpu_scalar_mul import _all_pairs
dev.init(0)
n = 0
for curve in (0, 1, 2, 3, 4):
    prs = _all_pairs(curve)
    s, p, z = sc.pack(curve, prs)
    out, oz = api.curve_scalar_mul(curve, s, p, z)
    sc.check(curve, prs, out, oz)
    n += len(prs)
print("CHECKED cases", n)
'''


def test_scalar_mul_through_the_checked_build():
    """The same cases through the checked build (tests/checked_child.py: a process of its own).  The kernels of scalar_mul.hip index
    no table - addends are selected by value from registers - so the guard counters have nothing of theirs to count; they must still
    all be zero."""
    assert "CHECKED cases" in checked_child.run_checked(CHECKED_BODY)


# ---- halo_n and halo_n_mul ----
def _halo_bits(curve):
    return (2, 4, 126, 128, br.CURVES[curve].scalar.bits & ~1)


@pytest.mark.parametrize("curve", he.ENDO_CURVES)
def test_halo_n_matches_the_restatement(curve):
    _dev()
    from plonky_amd import api
    f = br.CURVES[curve].scalar
    for bits in _halo_bits(curve):
        pats = he.chunk_patterns(bits, seed=20 + curve)
        # the same strings with the bits above security_bits set (they are ignored): all of them below the top bit, so the value stays below r
        high = [(v | (((1 << (f.bits - 1)) - 1) & ~((1 << bits) - 1))) for v in pats]
        vals = pats + [v for v in high if v < f.p]
        assert bits >= 250 or len(vals) > len(pats)
        if bits == 128:
            vals += sc.random_scalars(curve, 300 + curve, 256)
        got = _ints(f, api.halo_n(curve, _mont(f, vals), security_bits=bits))
        assert got == [he.halo_n(curve, he.bits_of(v, bits)) for v in vals], (curve, bits)


@pytest.mark.parametrize("curve", he.ENDO_CURVES)
def test_halo_n_mul_matches_algorithm_1_and_scalar_mul(curve):
    """[n(s)] P by Algorithm 1 against the restatement, and against scalar_mul(halo_n(s), P) on the device alone (the check that the
    ZETA of the addend and the ZETA_SCALAR of n(s) are one pair), P in {G, a seeded multiple, the identity}.

    A bit string that drives Acc through O or makes 2 Acc equal the next addend or its negative does not exist at these lengths: after
    j chunks Acc = [a zeta + b] P with |a|, |b| < 2^j, and 2 Acc = +-S or Acc = O would make (2b -+ 1, 2a), (2b, 2a -+ 1) or (b, a) a
    non-zero vector of the lattice {(u, v): u + v zeta = 0 mod r} with entries below 2^(j + 1); its shortest vector has entries near
    2^127 (GLV_BITS), so none exists for j <= 125, and for the last chunks of the 254-bit strings finding one is a lattice
    problem of its own - the case is dropped.  The first step (Acc = O) and the identity P run the same complete law here, and
    the shared group law's Acc = +-S branches are covered on chosen operands by tests/test_gpu_group_law.py."""
    _dev()
    from plonky_amd import api
    c = br.CURVES[curve]
    f = c.scalar
    G = (c.gx, c.gy)
    pts = [G, br.ec_mul(c, 0xFACADE + curve, G), None]
    for bits in _halo_bits(curve):
        pats = he.chunk_patterns(bits, seed=30 + curve)  # every chunk value in the first, a middle and the last chunk, at every length
        prs = [(v, P) for v in pats for P in pts]
        s, p, z = sc.pack(curve, prs)
        out, oz = api.halo_n_mul(curve, s, p, z, security_bits=bits)
        exp = sc.expect(curve, [he.halo_n_mul(curve, he.bits_of(v, bits), P) if P else None for v, P in prs])
        assert np.array_equal(oz, exp[1]) and np.array_equal(out, exp[0]), (curve, bits)
        out2, oz2 = api.curve_scalar_mul(curve, api.halo_n(curve, s, security_bits=bits), p, z)
        assert np.array_equal(oz, oz2) and np.array_equal(out, out2), (curve, bits)


def test_halo_entries_refuse_bls12_377_on_the_device():
    _dev()
    from plonky_amd import api
    c = br.BLS12_377
    s, p = _mont(c.scalar, [5]), _pt(2, (c.gx, c.gy))
    with pytest.raises(ValueError, match="endomorphism"):
        api.halo_n(2, s)
    with pytest.raises(ValueError, match="endomorphism"):
        api.halo_n_mul(2, s, p)


# ---- verification ----
def _prove(curve, n, freeze_log, seed):
    """One argument run round by round on the device; returns everything verify_ipa takes, as the interface's arrays."""
    dev = _dev()
    from plonky_amd import api
    c = br.CURVES[curve]
    f = c.scalar
    r = f.p
    G = (c.gx, c.gy)
    rounds = n.bit_length() - 1
    rnd = iter(sc.random_scalars(curve, seed, n + 3 * rounds + 8))
    a = [next(rnd) for _ in range(n)]
    x = next(rnd)
    b = [pow(x, i, r) for i in range(n)]
    rho, d, s_nonce, chall = next(rnd), next(rnd), next(rnd), next(rnd)
    us = [next(rnd) or 1 for _ in range(rounds)]
    blind = [(next(rnd), next(rnd)) for _ in range(rounds)]
    h, up = _pt(curve, br.ec_mul(c, 0xABCDEF01 + seed, G)), _pt(curve, br.ec_mul(c, 0x13579BDF + seed, G))
    g = dev.gen_bases_dev(curve, n, _pt(curve, G), _pt(curve, br.ec_mul(c, 0x9E3779B9 + seed, G)))
    g_host = dev.to_host(g)
    one = lambda v: _mont(f, [v])[0]
    commitment = api.msm_parallel(curve, _mont(f, a + [rho]), np.concatenate([g_host, h.reshape(1, 2, -1)]), 8)  # C = <a, G> + [rho] H
    value = sum(ai * bi for ai, bi in zip(a, b)) % r
    arg = dev.HaloArgument(curve, dev.to_device(_mont(f, a)), dev.to_device(_mont(f, b)), g, h, up, freeze_log=freeze_log)
    ls, rs, lz, rz = [], [], [], []
    randomness = rho
    for j in range(rounds):
        lr, z = arg.round_lr(one(blind[j][0]), one(blind[j][1]))
        ls.append(lr[0]); rs.append(lr[1]); lz.append(z[0]); rz.append(z[1])
        u = us[j]
        arg.round_fold(one(u), one(pow(u, -1, r)))
        randomness = (randomness + u * u * blind[j][0] + pow(u, -2, r) * blind[j][1]) % r       # halo.rs:107-109
    fa, fb, fg, fgz = arg.read()
    arg.free()
    assert fa.shape[0] == 1
    proof = api.schnorr_protocol(curve, fa[0], fb[0], (fg[0], fgz[0]), one(randomness), up, h, one(d), one(s_nonce), one(chall))
    L = c.base.n_limbs
    return dict(halo_l=(np.array(ls).reshape(rounds, 2, L), np.array(lz, dtype=np.uint8)), halo_r=(np.array(rs).reshape(rounds, 2, L), np.array(rz, dtype=np.uint8)),
                halo_g=(fg[0], int(fgz[0])), commitment=commitment, value=one(value), halo_b=fb[0], halo_us=_mont(f, us), u_prime=up, pedersen_h=h,
                schnorr_challenge=one(chall), schnorr_proof=proof), dict(x=x, us=us, g_host=g_host, fa=fa[0], value=value, a=a)


@pytest.mark.parametrize("curve", (0, 1, 3), ids=("Tweedledee", "Tweedledum", "Pallas"))
@pytest.mark.parametrize("n,freeze_log", [(2, 0), (16, 0), (64, 0), (256, 0), (256, 5)])
def test_the_provers_argument_verifies(curve, n, freeze_log):
    _dev()
    from plonky_amd import api
    c = br.CURVES[curve]
    f = c.scalar
    kw, extra = _prove(curve, n, freeze_log, 8000 + 13 * n + freeze_log)
    assert api.verify_ipa(curve, **kw) is True
    one = lambda v: _mont(f, [v])[0]
    assert not api.verify_ipa(curve, **dict(kw, value=one(extra["value"] + 1)))
    l_pts, l_zero = kw["halo_l"]
    neg = l_pts.copy()
    neg[0] = _pt(curve, br.ec_neg(c, _to_point(curve, l_pts[0], l_zero[0])))
    assert not api.verify_ipa(curve, **dict(kw, halo_l=(neg, l_zero)))
    r_pt, z1, z2 = kw["schnorr_proof"]
    assert not api.verify_ipa(curve, **dict(kw, schnorr_proof=(r_pt, one(_ints(f, z1)[0] + 1), z2)))
    if n > 2:
        assert not api.verify_ipa(curve, **dict(kw, halo_us=kw["halo_us"][::-1].copy()))
    # the prover's final b is g(x, us), and its final G is <halo_s(us), G>
    assert _ints(f, api.halo_g(f.field_id, one(extra["x"]), kw["halo_us"])) == _ints(f, kw["halo_b"])
    assert _ints(f, kw["halo_b"])[0] == he.halo_g(f.p, extra["x"], extra["us"])
    tables = api.msm_precompute(curve, extra["g_host"], 8)
    try:
        assert api.verify_halo_g(curve, kw["halo_g"], kw["halo_us"], tables)
        moved = br.ec_add(c, _to_point(curve, *kw["halo_g"]), _to_point(curve, extra["g_host"][0], 0))
        assert not api.verify_halo_g(curve, sc.point_limbs(curve, moved), kw["halo_us"], tables)
    finally:
        tables.free()


def test_verify_ipa_agrees_with_the_restatement():
    """the same proof through tests/halo_endo_ref.verify_ipa on integers: accepted as it is, refused with a changed value"""
    curve, n = 0, 16
    c = br.CURVES[curve]
    f = c.scalar
    kw, extra = _prove(curve, n, 0, 8100)
    pts = lambda arr, zero: [_to_point(curve, xy, z) for xy, z in zip(arr, zero)]
    r_pt, z1, z2 = kw["schnorr_proof"]
    args = [pts(*kw["halo_l"]), pts(*kw["halo_r"]), _to_point(curve, *kw["halo_g"]), _to_point(curve, *kw["commitment"]), extra["value"],
            _ints(f, kw["halo_b"])[0], extra["us"], _to_point(curve, kw["u_prime"], 0), _to_point(curve, kw["pedersen_h"], 0),
            _ints(f, kw["schnorr_challenge"])[0], (_to_point(curve, *r_pt), _ints(f, z1)[0], _ints(f, z2)[0])]
    assert he.verify_ipa(curve, *args)
    args[4] += 1
    assert not he.verify_ipa(curve, *args)


def test_u_prime_from_the_library_opens_the_tabled_argument():
    """u_prime = halo_n_mul(u_scaling, U) and u_prime_scalar = halo_n(u_scaling) from the library, fed to plk_halo_begin_tabled_dev with
    H and U inside the tables, give the L_j, R_j of the run with a host-computed u_prime (big integers, no scalar handed over)."""
    dev = _dev()
    from plonky_amd import api
    curve, n, seed = 0, 64, 9100
    c = br.CURVES[curve]
    f = c.scalar
    G = (c.gx, c.gy)
    L = c.base.n_limbs
    rounds = n.bit_length() - 1
    rnd = sc.random_scalars(curve, seed, 2 * n + 3 * rounds + 1)
    a, b, u_scaling = _mont(f, rnd[:n]), _mont(f, rnd[n:2 * n]), rnd[2 * n]
    us, bl = rnd[2 * n + 1:2 * n + 1 + rounds], _mont(f, rnd[2 * n + 1 + rounds:])
    U = br.ec_mul(c, 0x2468ACE + seed, G)
    h = _pt(curve, br.ec_mul(c, 0xABCDEF01 + seed, G))
    g = dev.gen_bases_dev(curve, n, _pt(curve, G), _pt(curve, br.ec_mul(c, 0x9E3779B9 + seed, G)))
    up_lib, upz = api.halo_n_mul(curve, _mont(f, [u_scaling]), _pt(curve, U))
    x_lib = api.halo_n(curve, _mont(f, [u_scaling]))[0]
    up_host = _pt(curve, br.ec_mul(c, he.halo_n(curve, he.bits_of(u_scaling, 128)), U))
    assert int(upz[0]) == 0 and np.array_equal(up_lib[0], up_host)
    tables = dev.msm_precompute_dev(curve, dev.to_device(np.concatenate([dev.to_host(g), h.reshape(1, 2, L), _pt(curve, U).reshape(1, 2, L)])))

    def run(u_prime, **kw):
        arg = dev.HaloArgument(curve, dev.to_device(a), dev.to_device(b), g, h, u_prime, freeze_log=3, tables=tables if kw else None, **kw)
        out = []
        for j in range(rounds):
            lr, z = arg.round_lr(bl[2 * j], bl[2 * j + 1])
            out.append((lr.copy(), np.array(z)))
            arg.round_fold(_mont(f, [us[j]])[0], _mont(f, [pow(us[j], -1, f.p)])[0])
        arg.free()
        return out

    with_lib = run(up_lib[0], h_index=n, u_index=n + 1, u_prime_scalar=x_lib)
    with_host = run(up_host)
    for j, ((lr1, z1), (lr2, z2)) in enumerate(zip(with_lib, with_host)):
        assert np.array_equal(lr1, lr2) and np.array_equal(z1, z2), "round %d" % j
