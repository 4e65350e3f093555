"""CPU-only: plonky_amd/csrc/h2c_step.cuh (the BLAKE3 block and blake_field, the code the kernels of hash_to_curve.hip run) compiled for
the host by tests/hash_to_curve_host_replay.cpp and compared with tests/hash_to_curve_ref.py, and both held to three published BLAKE3
digests.  The program is built a second time under AddressSanitizer + UBSan and run on its own (a stand-alone program: nothing of
it is loaded into Python).  The reference's own points are checked against the curve equation in Python integers, and the small seed
sets the GPU tests use are shown to reach every branch: a first try that succeeds, a third or later try, a hash that is not below the
modulus, and both values of y_neg."""
import pytest

from oracle import bigint_ref as br
from tests import hash_to_curve_ref as h2c
from tests import hostprog

SRC = "tests/hash_to_curve_host_replay.cpp"
# the BLAKE3 test vectors: the hash of the empty input, bytes 32..63 of its extended output (output words 8..15: where byte BYTES of
# every field and bytes 32..48 of Bls12377Base come from), and the hash of "abc"
DIGEST_EMPTY = "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262"
XOF_EMPTY_32_63 = "e00f03e7b69af26b7faaf09fcd333050338ddfe085b8cc869ca98b206c08243a"
DIGEST_ABC = "6437b3ac38465133ffb63b75273a8db548c558465d79db03fd359c6cd5bd9d85"
SEEDS = range(64)  # wide enough on every curve: test_small_seed_sets_reach_every_branch


def build_cases():
    """(field, seed, iter): edge seeds and small integers on all six fields, iters over the whole u8 range"""
    cases = []
    for field, f in sorted(br.FIELDS.items()):
        edge = [0, 1, f.p - 1, (1 << 64) - 1, (1 << 128) - 1, (1 << (f.bits - 1)) - 1, (1 << 32) + 7]
        for n, seed in enumerate(edge + list(range(2, 26))):
            cases.append((field, seed, (0, 1, 2, 7, 128, 255)[n % 6]))
    return cases


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("h2c")
    cases = build_cases()
    inp = str(tmp / "cases.txt")
    with open(inp, "w") as fh:
        for field, seed, it in cases:
            fh.write("%d %0*x %d\n" % (field, 16 * br.FIELDS[field].n_limbs, seed, it))
    return cases, hostprog.run(hostprog.build(SRC, tmp, hostprog.PLAIN, extra=("-Wall",)), inp), inp, tmp


def test_python_block_reproduces_the_published_digests():
    assert h2c.blake3_xof64(b"")[:32].hex() == DIGEST_EMPTY
    assert h2c.blake3_xof64(b"")[32:].hex() == XOF_EMPTY_32_63
    assert h2c.blake3_xof64(b"abc")[:32].hex() == DIGEST_ABC


def test_header_block_reproduces_the_published_digests(replayed):
    assert replayed[1].split("\n")[:3] == [DIGEST_EMPTY, XOF_EMPTY_32_63, DIGEST_ABC]


def test_header_blake_field_matches_the_reference_on_all_six_fields(replayed):
    cases, text = replayed[:2]
    lines = text.split("\n")[3:3 + len(cases)]
    assert len(lines) == len(cases)
    seen_j, seen_fields = 0, set()
    for (field, seed, it), line in zip(cases, lines):
        x, y_neg, j = h2c.blake_field(field, it, seed)
        width = 16 * br.FIELDS[field].n_limbs
        assert line == "%d %0*x %d 1 %0*x %d %d" % (field, width, seed, it, width, x, y_neg, j), (field, seed, it)
        seen_j += j > 0
        seen_fields.add(field)
    assert seen_fields == set(range(6)) and seen_j >= 6
    # the 50-byte message and the 7-bit shift of Bls12377Base, and a case that needed a second hash, are in the set
    assert any(f == 3 and h2c.blake_field(f, it, s)[2] > 0 for f, s, it in cases)
    assert any(f == 0 and h2c.blake_field(f, it, s)[2] > 0 for f, s, it in cases)


def test_replay_under_the_sanitizers(replayed):
    _, plain, inp, tmp = replayed
    sanitized = hostprog.run(hostprog.build(SRC, tmp, hostprog.ASAN_UBSAN, extra=("-Wall",)), inp)
    assert sanitized == plain


@pytest.mark.parametrize("curve", sorted(br.CURVES))
def test_reference_points_are_on_the_curve(curve):
    c = br.CURVES[curve]
    for seed in SEEDS:
        x, y, _, _ = h2c.hash_usize_to_curve(curve, seed)
        assert 0 <= x < c.base.p and 0 <= y < c.base.p and (y * y - x * x * x - c.b) % c.base.p == 0, seed


@pytest.mark.parametrize("curve", sorted(br.CURVES))
def test_small_seed_sets_reach_every_branch(curve):
    paths = [h2c.hash_usize_to_curve(curve, seed) for seed in SEEDS]
    y_negs = {h2c.blake_field(br.CURVES[curve].base.field_id, i, seed)[1] for seed, (_, _, i, _) in zip(SEEDS, paths)}
    assert any(i == 0 for _, _, i, _ in paths)
    assert any(i >= 2 for _, _, i, _ in paths)
    assert any(j >= 1 for _, _, _, j in paths)
    assert y_negs == {0, 1}
