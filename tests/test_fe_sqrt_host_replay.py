"""CPU-only: plonky_amd/csrc/fe_sqrt.cuh (fe_sqrt_with, the Tonelli-Shanks loop of the point decompression and of the two hashes to the
curve) compiled for the host by tests/fe_sqrt_host_replay.cpp and compared with the restatement of tests/sqrt_cases.py on the whole
case table of a 4-limb field with the deepest 2-adicity (Bls12377Scalar, 47), of the shallowest (PallasBase, 32) and of the 6-limb
field (Bls12377Base, 46): every depth of the loop, alone and in descending runs, b = 1 at entry, the non-residue exit and a = 0, through
the squarings and through a table indexed as SqrtRootFromTable indexes it.  The program is built a second time
under AddressSanitizer + UBSan and run on its own (a stand-alone program: nothing of it is loaded into Python)."""
import pytest

from oracle import bigint_ref as br
from tests import hostprog
from tests import sqrt_cases as sc

SRC = "tests/fe_sqrt_host_replay.cpp"
FIELDS = (br.BLS12_377_SCALAR, br.PALLAS_BASE, br.BLS12_377_BASE)


def hexm(f, x):  # canonical integer -> Montgomery words, most significant first
    return "%0*x" % (16 * f.n_limbs, f.to_mont(x % f.p))


def build_cases():
    """(input line, expected line, intended walk) of every case"""
    cases = []
    for f in FIELDS:
        none = "f" * (16 * f.n_limbs)
        for label, a, ks in sc.build_cases(f):
            root, walked = sc.restated_sqrt(f, a)
            assert (root is None) == (ks is None) and (ks is None or walked == ks), label
            half = "0 %s" % none if root is None else "1 %s" % hexm(f, root)
            cases.append(("Q %d %s" % (f.field_id, hexm(f, a)), "Q %d %s %s" % (f.field_id, half, half), ks))
    return cases


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fe_sqrt")
    cases = build_cases()
    inp = str(tmp / "cases.txt")
    with open(inp, "w") as fh:
        for line, _, _ in cases:
            fh.write(line + "\n")
    plain = hostprog.run(hostprog.build(SRC, tmp, hostprog.PLAIN, extra=("-Wall",)), inp)
    lines = plain.strip().split("\n")
    assert len(lines) == len(cases)
    return cases, lines, plain, inp, tmp


def test_header_roots_match_the_restatement_at_every_depth(replayed):
    cases, lines = replayed[:2]
    for (line, want, ks), got in zip(cases, lines):
        assert got == want, (line[:40], ks)
    # what the table claims to reach was reached: each field's deepest single step, its longest walk, both exits
    for f in FIELDS:
        mine = [ks for line, _, ks in cases if line.startswith("Q %d " % f.field_id)]
        assert [f.two_adicity - 1] in mine and list(range(f.two_adicity - 1, 0, -1)) in mine and [] in mine and None in mine


def test_header_squarings_and_table_give_the_same_bits(replayed):
    for got in replayed[1]:
        _, _, ok0, r0, ok1, r1 = got.split()
        assert (ok0, r0) == (ok1, r1), got


def test_replay_under_the_sanitizers(replayed):
    _, _, plain, inp, tmp = replayed
    sanitized = hostprog.run(hostprog.build(SRC, tmp, hostprog.ASAN_UBSAN, extra=("-Wall",)), inp)
    assert sanitized == plain
