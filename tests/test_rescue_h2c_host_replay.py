"""CPU-only: plonky_amd/csrc/rescue_h2c_step.cuh (the seed formation, the y_neg bit, one try and the bounded loop over the tries - the
code k_rescue_h2c_tries runs) compiled for the host by tests/rescue_h2c_host_replay.cpp and compared with tests/rescue_h2c_ref.py on a
4-limb field (TweedledeeBase, under Tweedledee) and on the 6-limb field (Bls12377Base, under BLS12-377).  The program is built a
second time under AddressSanitizer + UBSan and run on its own (a stand-alone program: nothing of it is loaded into Python).

The try limit is a parameter of the step, so a limit of one or two tries reaches the status-2 path that no real input reaches at 256."""
import pytest

from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from tests import hostprog
from tests import rescue_h2c_ref as ref
from tests import rescue_ref as rr

SRC = "tests/rescue_h2c_host_replay.cpp"
CURVES = (0, 2)  # base fields 0 (4 limbs) and 3 (6 limbs)
ROUNDS = {0: (2, 16), 2: (2,)}
SEEDS = list(range(12)) + [(1 << 32) - 1, 1 << 32, (1 << 64) - 1]
U64S = (0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 63) + 5, (1 << 64) - 1)


def hexm(f, x):  # canonical integer -> Montgomery words, most significant first
    return "%0*x" % (16 * f.n_limbs, f.to_mont(x % f.p))


def build_cases():
    """(kind, curve, ...) with the expected line of each"""
    cases = []
    for curve in CURVES:
        c = br.CURVES[curve]
        f = c.base
        fid = f.field_id
        for n in U64S:
            cases.append(("S %d %d" % (fid, n), "S %d %s" % (fid, hexm(f, n))))
        for v in (0, 1, 2, f.p - 1, f.p - 2, 1 << 64, (1 << 64) + 1) + tuple(f.from_mont(br.limbs_to_int(l)) for l in br.rand_field_limbs(f, 0x2E6 + fid, 6)):
            cases.append(("Y %d %s" % (fid, hexm(f, v)), "Y %d %d" % (fid, v & 1)))
        for rounds in ROUNDS[curve]:
            consts = rr.constants(fid, 4, rounds)
            cw = " ".join(hexm(f, v) for a, b in consts for v in a + b)
            seeds = SEEDS if rounds == 2 else SEEDS[:3]
            p_seed = f.p - 1
            for seed in seeds + [p_seed]:
                x, y, t = ref.hash_base_field_to_curve(curve, seed, consts, key=("replay", rounds))
                point = "%s %s" % (hexm(f, x), hexm(f, y))
                none = "%s %s" % (hexm(f, 0), hexm(f, 0))

                def case(i_first, i_last, found):
                    cases.append(("T %d %d %d %d %d %s %s" % (fid, c.b, rounds, i_first, i_last, cw, hexm(f, seed)),
                                  "T %d %d %s" % (fid, 0 if found else 2, point if found else none)))
                case(0, 255, True)
                for limit in (1, 2):  # tries 0 .. limit - 1
                    case(0, limit - 1, t < limit)
                for i in range(t + 1):  # one try at a time: every i below t fails, t gives the point
                    case(i, i, i == t)
                if t > 0:
                    case(t, 255, True)  # the tail of the rounds: entering at the try that settles
    return cases


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    ol.build()
    tmp = tmp_path_factory.mktemp("rescue_h2c")
    cases = build_cases()
    inp = str(tmp / "cases.txt")
    with open(inp, "w") as fh:
        for line, _ in cases:
            fh.write(line + "\n")
    plain = hostprog.run(hostprog.build(SRC, tmp, hostprog.PLAIN, extra=("-Wall",)), inp)
    lines = plain.strip().split("\n")
    assert len(lines) == len(cases)
    return cases, lines, plain, inp, tmp


def _compare(replayed, kind):
    cases, lines = replayed[:2]
    n = 0
    for (line, want), got in zip(cases, lines):
        if line[0] == kind:
            assert got == want, line[:60]
            n += 1
    return n


def test_header_seed_formation_is_from_canonical_u64(replayed):
    assert _compare(replayed, "S") == len(CURVES) * len(U64S)


def test_header_y_neg_is_bit_zero_of_the_canonical_form(replayed):
    cases = replayed[0]
    assert _compare(replayed, "Y") == len(CURVES) * 13
    assert {want[-1] for line, want in cases if line[0] == "Y"} == {"0", "1"}


def test_header_tries_match_the_restatement_and_the_limit_gives_status_two(replayed):
    cases = replayed[0]
    assert _compare(replayed, "T") > 100
    wants = [want.split() for line, want in cases if line[0] == "T"]
    assert sum(w[2] == "2" for w in wants) > 20 and sum(w[2] == "0" for w in wants) > 60  # both paths were walked
    for w in wants:
        assert (w[2] == "2") == (int(w[3], 16) == 0 and int(w[4], 16) == 0)


def test_replay_under_the_sanitizers(replayed):
    _, _, plain, inp, tmp = replayed
    sanitized = hostprog.run(hostprog.build(SRC, tmp, hostprog.ASAN_UBSAN, extra=("-Wall",)), inp)
    assert sanitized == plain
