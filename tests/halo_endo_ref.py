"""A restatement on integers of the reference's Halo endomorphism arithmetic and IPA verifier, written from its text:
halo_n / halo_n_mul (plonk_util.rs:50-110), halo_g (plonk_util.rs:329-339), schnorr_protocol and verify_ipa (halo.rs:157-223).
Points are oracle.bigint_ref's (x, y) / None; scalars are canonical integers.  The ZETA / ZETA_SCALAR limbs are the reference's
Montgomery-form constants (tweedledee_curve.rs:22-37 and its three siblings), typed in as data."""
from oracle import bigint_ref as br

# curve id -> (ZETA limbs in the base field, ZETA_SCALAR limbs in the scalar field), Montgomery form, least significant first
_ZETA_LIMBS = {
    0: ([1444470991491022206, 3301226169728360777, 72516509137424193, 708688398506307241],
        [13597504620482004229, 16590497220115833568, 15137822970486674306, 1901757351910266741]),
    1: ([7605997034305223424, 3132214451552427455, 3308921103222877309, 2709928666517121162],
        [9282944046338294407, 16421485501699768486, 18374227564572127422, 3902997619921080662]),
    3: ([0xfbdfd7aa9e65eac8, 0x0cd4d654e50025fb, 0xd59892a33785b99a, 0x2a27fb62585e8789],
        [0x410e7d207feeeee3, 0x6afdf14fd8fa2279, 0xfd3d8a04eca4d4d7, 0x2de2d60777dba4ef]),
    4: ([0x410e7d207feeeee3, 0x6afdf14fd8fa2279, 0xfd3d8a04eca4d4d7, 0x2de2d60777dba4ef],
        [0xfbdfd7aa9e65eac8, 0x0cd4d654e50025fb, 0xd59892a33785b99a, 0x2a27fb62585e8789]),
}
ENDO_CURVES = tuple(sorted(_ZETA_LIMBS))


def zeta(curve):  # HaloCurve::ZETA, canonical
    return br.CURVES[curve].base.from_mont(br.limbs_to_int(_ZETA_LIMBS[curve][0]))


def zeta_scalar(curve):  # HaloCurve::ZETA_SCALAR, canonical
    return br.CURVES[curve].scalar.from_mont(br.limbs_to_int(_ZETA_LIMBS[curve][1]))


def bits_of(s, security_bits):
    """to_canonical_bool_vec()[..security_bits] (field.rs:104-112): least significant bit first."""
    return [(s >> i) & 1 for i in range(security_bits)]


def halo_n(curve, s_bits):
    assert len(s_bits) % 2 == 0
    r = br.CURVES[curve].scalar.p
    a = b = 0
    for i in range(0, len(s_bits), 2):
        bit_lo, bit_hi = s_bits[i], s_bits[i + 1]
        sign = 1 if bit_lo else r - 1
        c, d = (sign, 0) if bit_hi else (0, sign)
        a = (2 * a + c) % r
        b = (2 * b + d) % r
    return (a * zeta_scalar(curve) + b) % r


def endomorphism(curve, P):  # curve.rs:140-149
    return None if P is None else (zeta(curve) * P[0] % br.CURVES[curve].base.p, P[1])


def halo_n_mul(curve, s_bits, P, trace=None):
    """Algorithm 1 as plonk_util.rs:79-110 restates it; trace (a list) receives (Acc before the step, addend) pairs."""
    assert len(s_bits) % 2 == 0
    c = br.CURVES[curve]
    p_p, p_n = P, br.ec_neg(c, P)
    e_p = endomorphism(curve, P)
    e_n = br.ec_neg(c, e_p)
    acc = None
    for i in range(0, len(s_bits), 2):
        bit_lo, bit_hi = s_bits[i], s_bits[i + 1]
        s = (e_p if bit_lo else e_n) if bit_hi else (p_p if bit_lo else p_n)
        dbl = br.ec_add(c, acc, acc)
        if trace is not None:
            trace.append((dbl, s))
        acc = br.ec_add(c, dbl, s)
    return acc


def halo_g(p, x, us):
    product, x_power = 1, x
    for u in reversed(us):
        product = product * (u * x_power + pow(u, -1, p)) % p
        x_power = x_power * x_power % p
    return product


def fold_b(p, b, u):  # halo.rs:118: halo_b = u^-1 b_lo + u b_hi
    m = len(b) // 2
    ui = pow(u, -1, p)
    return [(ui * b[i] + u * b[m + i]) % p for i in range(m)]


def schnorr_protocol(curve, halo_a, halo_b, halo_g_pt, randomness, u_prime, pedersen_h, d, s, chall):
    c = br.CURVES[curve]
    r = c.scalar.p
    r_curve = br.ec_add(c, br.ec_mul(c, d, br.ec_add(c, halo_g_pt, br.ec_mul(c, halo_b, u_prime))), br.ec_mul(c, s, pedersen_h))
    return r_curve, (halo_a * chall + d) % r, (randomness * chall + s) % r


def verify_ipa(curve, halo_l, halo_r, halo_g_pt, commitment, value, halo_b, halo_us, u_prime, pedersen_h, schnorr_challenge, schnorr_proof):
    c = br.CURVES[curve]
    r = c.scalar.p
    p_prime = br.ec_add(c, commitment, br.ec_mul(c, value, u_prime))
    scalars = [u * u % r for u in halo_us] + [pow(u, -2, r) for u in halo_us]
    q = br.ec_add(c, br.msm(c, scalars, list(halo_l) + list(halo_r)), p_prime)
    r_pt, z1, z2 = schnorr_proof
    lhs = br.ec_add(c, br.ec_mul(c, schnorr_challenge, q), r_pt)
    rhs = br.ec_add(c, br.ec_mul(c, z1, br.ec_add(c, halo_g_pt, br.ec_mul(c, halo_b, u_prime))), br.ec_mul(c, z2, pedersen_h))
    return lhs == rhs


def chunk_patterns(security_bits, seed=1):
    """Bit strings (as integers below 2^security_bits) that put each of the four chunk values into the first, a middle and the last
    chunk of a seeded background, plus the all-zeros and all-ones strings."""
    gen = br.splitmix64_stream(seed)
    base = 0
    for i in range(4):
        base |= next(gen) << (64 * i)
    base &= (1 << security_bits) - 1
    chunks = security_bits // 2
    out = [0, (1 << security_bits) - 1]
    for pos in sorted({0, chunks // 2, chunks - 1}):
        for v in range(4):
            out.append((base & ~(3 << (2 * pos))) | (v << (2 * pos)))
    return out
