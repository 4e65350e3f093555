"""Inputs to Field::square_root (field.rs:440-472) chosen by the walk they make Tonelli-Shanks take, on Python integers alone.

For a field p with A = TWO_ADICITY, T = (p - 1) >> A (odd), zeta = g^T (the 2^A-th root of unity the loop starts from) and any h,

    a = zeta^e * h^(2^A),   e = d * T^-1 mod 2^A,        has        b = a^T = zeta^d * h^(p - 1) = zeta^d,

so d alone dictates the loop.  One step: with v2 = the number of trailing zero bits of d (mod 2^A), b has order 2^k for k = A - v2; the step
multiplies b by z = zeta^(2^(A - k)) = zeta^(2^v2), i.e. d becomes d + 2^v2 (mod 2^A), and the loop ends at d = 0.  `walk(A, d)` is that
rule: pure 2-adic arithmetic, no field operation - the INTENDED list of k.  An odd d gives k = A at the first step: a non-residue.

  d = 2^A - 2^(A - k)     ONE step at depth k (d + 2^(A - k) = 0), for every k in 1 .. A - 1, the deepest included
  d = 2^(A - k)           k, k - 1, ..., 1: a descending run that STARTS at depth k, for every k in 1 .. A - 1; k = A - 1 (d = 2) is the
                          longest walk there is, every depth once
  d = 2^A - 2             one step at the deepest depth, A - 1 (the first family's last member, kept by name)
  0x5555.. and 0xAAAA..   truncated to A bits and to even: carries through every second bit
  d = 0                   b = 1 at entry, no step
  odd d                   1, 3, 2^A - 1, the odd 0x5555.. pattern, 2^(A-1) + 1: non-residues, refused at k >= v
and the fixed values 0, 1, p - 1, 4, the curve constants x^3 + B at x = 0 (5, 7, 1) and g itself, whose d comes from `two_adic_log`.

`restated_sqrt` is the reference's loop restated on integers; it returns the root and the list of k it walked.
"""
import random

from oracle import bigint_ref as br

FIELDS = [br.FIELDS[i] for i in sorted(br.FIELDS)]
H_PER_CASE = 3
CURVE_BS = (5, 7, 1)  # tweedledee / pallas / vesta, tweedledum, bls12-377


def zeta(f):
    return pow(f.generator, f.T, f.p)


def walk(A, d):
    """the k of every step of the loop for b = zeta^d; None for a non-residue (odd d)"""
    d %= 1 << A
    if d & 1:
        return None
    ks = []
    while d:
        v2 = (d & -d).bit_length() - 1
        ks.append(A - v2)
        d = (d + (1 << v2)) % (1 << A)
    return ks


def two_adic_log(f, b):
    """d with zeta^d = b for b in the 2^A-torsion, bit by bit from the bottom (Pohlig-Hellman)"""
    A, p = f.two_adicity, f.p
    z_inv = pow(zeta(f), -1, p)
    d = 0
    for i in range(A):
        if pow(b * pow(z_inv, d, p) % p, 1 << (A - 1 - i), p) != 1:
            d |= 1 << i
    assert pow(zeta(f), d, p) == b
    return d


def element(f, d, h):
    A, p = f.two_adicity, f.p
    e = d * pow(f.T, -1, 1 << A) % (1 << A)
    return pow(zeta(f), e, p) * pow(h, 1 << A, p) % p


def exponents(f):
    """(label, d) for the constructed cases of field f"""
    A = f.two_adicity
    full = (1 << A) - 1
    out = []
    for k in range(1, A):
        out.append(("one_step_k%d" % k, (1 << A) - (1 << (A - k))))
    for k in range(1, A):
        out.append(("descend_from_k%d" % k, 1 << (A - k)))
    out.append(("two_to_A_minus_2", (1 << A) - 2))
    out.append(("alt_5555", (int("5" * 16, 16) & full) & ~1))
    out.append(("alt_aaaa", (int("a" * 16, 16) & full) & ~1))
    out.append(("b_is_one", 0))
    for d in (1, 3, full, int("5" * 16, 16) & full | 1, (1 << (A - 1)) + 1):
        out.append(("odd_%x" % d, d))
    return out


def build_cases(f):
    """[(label, a, ks)]: a canonical, ks the intended walk (None: a non-residue), the same list on every call"""
    A, p = f.two_adicity, f.p
    rng = random.Random(0x5A27 + f.field_id)
    cases = []
    for label, d in exponents(f):
        for j in range(H_PER_CASE):
            cases.append(("%s_h%d" % (label, j), element(f, d, rng.randrange(1, p)), walk(A, d)))
    cases.append(("zero", 0, []))
    for label, a in [("one", 1), ("minus_one", p - 1), ("four", 4)] + [("b_%d" % b, b) for b in CURVE_BS] + [("generator", f.generator)]:
        cases.append((label, a % p, walk(A, two_adic_log(f, pow(a, f.T, p)))))
    return cases


def restated_sqrt(f, a):
    """field.rs:440-472 on canonical integers -> (root or None, the k of every step)"""
    p, A = f.p, f.two_adicity
    a %= p
    if a == 0:
        return 0, []
    if pow(a, (p - 1) // 2, p) != 1:  # is_quadratic_residue (field.rs:377-391): Euler's criterion
        return None, []
    z = pow(f.generator, f.T, p)
    w = pow(a, (f.T - 1) // 2, p)
    x = w * a % p
    b = x * w % p
    v = A
    ks = []
    while b != 1:
        k = 0
        b2k = b
        while b2k != 1:
            b2k = b2k * b2k % p
            k += 1
        ks.append(k)
        j = v - k - 1
        w = z
        for _ in range(j):
            w = w * w % p
        z = w * w % p
        b = b * z % p
        x = x * w % p
        v = k
    return x, ks
