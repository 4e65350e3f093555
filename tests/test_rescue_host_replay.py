"""CPU-only: plonky_amd/csrc/rescue_step.cuh (the exponent of a k-th root, the Cauchy matrix, the windowed power chain, the row sum
under one reduction and the round - the code the kernels of rescue.hip run) compiled for the host by tests/rescue_host_replay.cpp and
compared with tests/rescue_ref.py on all six fields.  The program is built a second time under AddressSanitizer + UBSan and run
on its own (a stand-alone program: nothing of it is loaded into Python)."""
import pytest

from oracle import bigint_ref as br
from tests import hostprog
from tests import rescue_ref as rr

SRC = "tests/rescue_host_replay.cpp"
KS = (0, 1, 2, 3, 5, 7, 11, 13, 17, 257, 65537, 1000003, 2 ** 31 - 1, 2 ** 32 - 1)
ROUNDS = (1, 2, 10)


def hexm(f, x):  # canonical integer -> Montgomery words, most significant first
    return "%0*x" % (16 * f.n_limbs, f.to_mont(x % f.p))


def root_inputs(f, field):
    return [0, 1, f.p - 1, 2] + [f.from_mont(br.limbs_to_int(l)) for l in br.rand_field_limbs(f, 7 + field, 2)]


def states(f, field):
    rnd = [f.from_mont(br.limbs_to_int(l)) for l in br.rand_field_limbs(f, 99 + field, 8)]
    return [[0] * 4, [f.p - 1] * 4, [1, 0, 0, 0], [0, 0, 0, 1], rnd[:4], rnd[4:]]


def build_cases():
    cases = []
    for field, f in sorted(br.FIELDS.items()):
        cases.append(("M", field))
        for k in KS:
            for x in root_inputs(f, field)[:6 if k in (1, 5, 11) else 2]:
                cases.append(("K", field, k, x))
        for rounds in ROUNDS:
            for st in states(f, field):
                cases.append(("P", field, rounds, st))
    return cases


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rescue")
    cases = build_cases()
    inp = str(tmp / "cases.txt")
    with open(inp, "w") as fh:
        for c in cases:
            f = br.FIELDS[c[1]]
            if c[0] == "M":
                fh.write("M %d\n" % c[1])
            elif c[0] == "K":
                fh.write("K %d %d %s\n" % (c[1], c[2], hexm(f, c[3])))
            else:
                consts = rr.constants(c[1], 4, c[2])
                words = [hexm(f, v) for a, b in consts for v in a + b] + [hexm(f, v) for v in c[3]]
                fh.write("P %d %d %s\n" % (c[1], c[2], " ".join(words)))
    plain = hostprog.run(hostprog.build(SRC, tmp, hostprog.PLAIN, extra=("-Wall",)), inp)
    lines = plain.strip().split("\n")
    assert len(lines) == len(cases)
    return cases, lines, plain, inp, tmp


def test_header_exponent_is_the_one_the_reference_walks_to(replayed):
    cases, lines = replayed[:2]
    seen_ok = seen_refused = 0
    for c, line in zip(cases, lines):
        if c[0] != "K":
            continue
        _, field, k, x = c
        f = br.FIELDS[field]
        # the walk over n is the reference's; for a large k its result is found the short way and checked by what defines it
        if k <= 65537:
            d = rr.kth_root_exponent(f.p, k) if k else None
        else:
            from math import gcd
            d = None
            if gcd(k, f.p - 1) == 1:
                m = (-pow((f.p - 1) % k, -1, k)) % k
                m += k if m < 2 else 0
                assert (m * (f.p - 1) + 1) % k == 0 and 2 <= m <= k + 1
                d = ((m * (f.p - 1) + 1) // k) % (f.p - 1)
        tok = line.split()
        width = 16 * f.n_limbs
        if d is None:
            assert tok == ["K", str(field), str(k), "0", "0" * width, "0" * width], c
            seen_refused += 1
        else:
            y = pow(x, d, f.p)
            assert pow(y, k, f.p) == x
            assert tok == ["K", str(field), str(k), "1", "%0*x" % (width, d), hexm(f, y)], c
            seen_ok += 1
    assert seen_ok > 100 and seen_refused > 20


def test_header_matrix_and_alpha(replayed):
    cases, lines = replayed[:2]
    n = 0
    for c, line in zip(cases, lines):
        if c[0] != "M":
            continue
        f = br.FIELDS[c[1]]
        want = ["M", str(c[1]), str(rr.ALPHA[c[1]])] + [hexm(f, v) for row in rr.mds_matrix(f.p, 4) for v in row]
        assert line.split() == want
        n += 1
    assert n == 6


def test_header_round_matches_the_reference_on_all_six_fields(replayed):
    cases, lines = replayed[:2]
    n = 0
    for c, line in zip(cases, lines):
        if c[0] != "P":
            continue
        _, field, rounds, st = c
        f = br.FIELDS[field]
        want = rr.rescue_permutation(field, st, rr.constants(field, 4, rounds))
        assert line.split() == ["P", str(field), str(rounds)] + [hexm(f, v) for v in want], c[:3]
        n += 1
    assert n == 6 * len(ROUNDS) * 6


def test_replay_under_the_sanitizers(replayed):
    _, _, plain, inp, tmp = replayed
    sanitized = hostprog.run(hostprog.build(SRC, tmp, hostprog.ASAN_UBSAN, extra=("-Wall",)), inp)
    assert sanitized == plain
