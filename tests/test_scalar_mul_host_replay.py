"""CPU-only: plonky_amd/csrc/scalar_mul_step.cuh (the chunk decoding and n(s), the signed-digit recoding, the split along the
endomorphism and the addend selections - the code the kernels of scalar_mul.hip run) compiled for the host by
tests/scalar_mul_host_replay.cpp and compared with tests/halo_endo_ref.py.  The program is built a second time
under AddressSanitizer + UBSan and run on its own (a stand-alone program: nothing of it is loaded into Python)."""
import pytest

from oracle import bigint_ref as br
from tests import hostprog
from tests import halo_endo_ref as he
from tests import scalar_mul_cases as sc

SRC = "tests/scalar_mul_host_replay.cpp"
GLV_BITS = 130  # glv_params.cuh


def hexm(f, x):  # canonical integer -> Montgomery words, most significant first
    return "%0*x" % (16 * f.n_limbs, f.to_mont(x % f.p))


def scalars(curve):
    r = br.CURVES[curve].scalar.p
    rnd = [br.limbs_to_int(l) % r for l in br.rand_field_limbs(br.CURVES[curve].scalar, 40 + curve, 6)]
    return [0, 1, 2, r - 1, r - 2, (r - 1) // 2, (1 << 128) - 1, 1 << 129, he.zeta_scalar(curve), r - he.zeta_scalar(curve)] + rnd


def digit_inputs():
    r = br.BLS12_377.scalar.p
    ones = (1 << 256) - 1
    out = [0, 1, 2, 3, r - 1, r - 2, ones, ones - 1, 3 << 254, 0xAAAA << 240, int("3" * 64, 16), int("2" * 64, 16), int("b" * 64, 16)]
    out += [(3 << (2 * j)) for j in (0, 15, 16, 63, 64, 126, 127)]            # an all-ones window at the word and limb boundaries
    out += [(1 << (2 * j)) - 1 for j in (1, 16, 17, 64, 127, 128)]            # runs of all-ones windows: the carry travels
    out += [br.limbs_to_int(l) for l in br.rand_field_limbs(br.BLS12_377.scalar, 9, 8)]
    return out


def build_cases():
    cases = []
    for curve in he.ENDO_CURVES:
        c = br.CURVES[curve]
        for bits in (2, 4, 126, 128, c.scalar.bits & ~1):
            for s in he.chunk_patterns(bits, seed=curve + 11)[:8] + [c.scalar.p - 1]:
                cases.append(("N", curve, bits, s % c.scalar.p))
        for s in scalars(curve):
            cases.append(("G", curve, s))
        for k in (1, 7):
            P = br.ec_mul(c, k, (c.gx, c.gy))
            cases.append(("A", curve, P))
            for n1 in (0, 1):
                for n2 in (0, 1):
                    cases.append(("S", curve, n1, n2, P))
    for k in digit_inputs():
        cases.append(("D", 2, k))
    # the chains the kernels run, step by step: every curve's scalar_mul (the base-4 walk on BLS12-377), Algorithm 1 at three lengths
    for curve in sorted(br.CURVES):
        c = br.CURVES[curve]
        r = c.scalar.p
        G = (c.gx, c.gy)
        P = br.ec_mul(c, 0xBADC0DE + curve, G)
        cases.append(("W", curve, P))
        ks = [0, 1, 2, 3, 4, r - 1, (r + 1) // 2, (1 << 128) - 1] + sc.random_scalars(curve, 60 + curve, 3)
        ks += sc.glv_edge_scalars(curve)[0][:4] if curve in he.ENDO_CURVES else [int("9" * 63, 16) % r, int("e" * 63, 16) % r]
        for k in ks:
            cases.append(("M", curve, k, P))
        if curve == 2:
            cases += [("M", 2, k, (c.base.p - 1, 0)) for k in (1, 2, 3, r - 1)]  # the 2-torsion point: 2P = O in the table
        else:
            for bits in (2, 128, c.scalar.bits & ~1):
                for s in he.chunk_patterns(bits, seed=curve + 5)[:4]:
                    cases.append(("H", curve, bits, s % r, P))
    return cases


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scalar_mul")
    cases = build_cases()
    inp = str(tmp / "cases.txt")
    with open(inp, "w") as fh:
        for c in cases:
            cv = br.CURVES[c[1]]
            if c[0] == "N":
                fh.write("N %d %d %s\n" % (c[1], c[2], hexm(cv.scalar, c[3])))
            elif c[0] == "G":
                fh.write("G %d %s\n" % (c[1], hexm(cv.scalar, c[2])))
            elif c[0] == "D":
                fh.write("D %d %064x\n" % (c[1], c[2]))
            elif c[0] == "W":
                fh.write("W %d %s %s\n" % (c[1], hexm(cv.base, c[2][0]), hexm(cv.base, c[2][1])))
            elif c[0] == "M":
                fh.write("M %d %s %s %s\n" % (c[1], hexm(cv.scalar, c[2]), hexm(cv.base, c[3][0]), hexm(cv.base, c[3][1])))
            elif c[0] == "H":
                fh.write("H %d %d %s %s %s\n" % (c[1], c[2], hexm(cv.scalar, c[3]), hexm(cv.base, c[4][0]), hexm(cv.base, c[4][1])))
            elif c[0] == "A":
                fh.write("A %d %s %s\n" % (c[1], hexm(cv.base, c[2][0]), hexm(cv.base, c[2][1])))
            else:
                fh.write("S %d %d %d %s %s\n" % (c[1], c[2], c[3], hexm(cv.base, c[4][0]), hexm(cv.base, c[4][1])))
    plain = hostprog.run(hostprog.build(SRC, tmp, hostprog.PLAIN, extra=("-Wall",)), inp)
    lines = plain.strip().split("\n")
    assert len(lines) == len(cases)
    return cases, lines, plain, inp, tmp


def test_chunks_and_halo_n(replayed):
    cases, lines = replayed[:2]
    n = 0
    for c, line in zip(cases, lines):
        if c[0] != "N":
            continue
        _, curve, bits, s = c
        sb = he.bits_of(s, bits)
        chunks = "".join(str(sb[2 * i] | sb[2 * i + 1] << 1) for i in range(bits // 2))
        assert line.split() == ["N", str(curve), str(bits), chunks, hexm(br.CURVES[curve].scalar, he.halo_n(curve, sb))], c
        n += 1
    assert n == sum(1 for c in cases if c[0] == "N") and n > 150


def test_signed_digits_sum_to_the_scalar(replayed):
    cases, lines = replayed[:2]
    carried = 0
    for c, line in zip(cases, lines):
        if c[0] != "D":
            continue
        tok = line.split()
        carry, digits = int(tok[2]), [int(t) for t in tok[3:]]
        assert len(digits) == 128 and all(-1 <= d <= 2 for d in digits) and carry in (0, 1)
        assert sum(d << (2 * j) for j, d in enumerate(digits)) + (carry << 256) == c[2], hex(c[2])
        if c[2] < (1 << 255):
            assert carry == 0          # every scalar field here: the walk needs no 129th digit
        if c[2] < br.BLS12_377.scalar.p:
            assert digits[127] == 0
        carried += carry
    assert carried >= 3                # inputs whose recoding carries out of the top window are among the cases


def test_glv_halves_recombine(replayed):
    cases, lines = replayed[:2]
    n = 0
    for c, line in zip(cases, lines):
        if c[0] != "G":
            continue
        _, curve, s = c
        r = br.CURVES[curve].scalar.p
        tok = line.split()
        squared, n1, k1, n2, k2 = int(tok[2]), int(tok[3]), int(tok[4], 16), int(tok[5]), int(tok[6], 16)
        assert squared == (1 if curve == 4 else 0)
        lam = pow(he.zeta_scalar(curve), 2 if squared else 1, r)  # the lattice's LAMBDA: ZETA_SCALAR, or its square where the pair differs
        assert k1 < (1 << GLV_BITS) and k2 < (1 << GLV_BITS)
        assert ((-k1 if n1 else k1) + (-k2 if n2 else k2) * lam - s) % r == 0, c
        want = sc.glv_split(curve, s)  # the restated split: the same two halves, sign for sign (a zero half carries no sign)
        assert (k1, k2) == (abs(want[0]), abs(want[1])) and (n1, n2) == (int(want[0] < 0), int(want[1] < 0)), c
        n += 1
    assert n == sum(1 for c in cases if c[0] == "G") and n >= 4 * 16


def test_addend_selection(replayed):
    cases, lines = replayed[:2]
    n = 0
    for c, line in zip(cases, lines):
        cv = br.CURVES[c[1]]
        f = cv.base
        tok = line.split()[2:]
        if c[0] in ("W", "M", "H"):
            continue
        if c[0] == "A":
            P = c[2]
            e = he.endomorphism(c[1], P)
            want = [br.ec_neg(cv, P), P, br.ec_neg(cv, e), e]  # chunk = bit_lo | bit_hi << 1 (plonk_util.rs:95-105)
            assert tok == [hexm(f, v) for pt in want for v in pt], c
            n += 1
        elif c[0] == "S":
            _, curve, n1, n2, P = c
            lam_pt = he.endomorphism(curve, he.endomorphism(curve, P)) if curve == 4 else he.endomorphism(curve, P)  # [LAMBDA] P of the lattice
            s1, s2 = (br.ec_neg(cv, P) if n1 else P), (br.ec_neg(cv, lam_pt) if n2 else lam_pt)
            want = [s1, s2, br.ec_add(cv, s1, s2)]
            assert tok == [hexm(f, v) for pt in want for v in pt], c
            n += 1
    assert n == 4 * 2 * 5


def _affine_tokens(curve, P):
    f = br.CURVES[curve].base
    return ["1", hexm(f, 0), hexm(f, 0)] if P is None else ["0", hexm(f, P[0]), hexm(f, P[1])]


def test_base4_addend_and_affine_doubling(replayed):
    cases, lines = replayed[:2]
    n = 0
    for c, line in zip(cases, lines):
        if c[0] != "W":
            continue
        cv = br.CURVES[c[1]]
        P = c[2]
        two = br.ec_add(cv, P, P)
        want = [two, br.ec_neg(cv, P), P, two]  # 2P, then the addends of d = -1, 1, 2
        assert line.split()[2:] == [hexm(cv.base, v) for pt in want for v in pt], c
        n += 1
    assert n == 5


def test_chains_step_by_step(replayed):
    """sm_scalar_mul_chain and halo_n_mul_chain - every chain step the kernels run, on the host - against big integers"""
    cases, lines = replayed[:2]
    n_m = n_h = 0
    for c, line in zip(cases, lines):
        tok = line.split()
        if c[0] == "M":
            _, curve, k, P = c
            assert tok[2:] == _affine_tokens(curve, br.ec_mul(br.CURVES[curve], k, P)), (curve, hex(k))
            n_m += 1
        elif c[0] == "H":
            _, curve, bits, s, P = c
            assert tok[3:] == _affine_tokens(curve, he.halo_n_mul(curve, he.bits_of(s, bits), P)), (curve, bits, hex(s))
            n_h += 1
    assert n_m >= 5 * 13 and n_h == 4 * 3 * 4


def test_replay_under_the_sanitizers(replayed):
    _, _, plain, inp, tmp = replayed
    sanitized = hostprog.run(hostprog.build(SRC, tmp, hostprog.ASAN_UBSAN, extra=("-Wall",)), inp)
    assert sanitized == plain
