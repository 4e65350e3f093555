"""GPU parity: the plain XYZZ law of ec.cuh (xyzz_madd, xyzz_mdbl, xyzz_dbl, xyzz_add, xyzz_to_affine) through the three kernels of
curve_ops.hip that are built on it, against big integers.

plk_curve_op never reaches this law (it runs ecz.cuh / ecz_coop.cuh), and the tests on random points reach its exceptional branches only
by chance.  tests/xyzz_cases.py places equal, opposite, flagged and 2-torsion points where the schedule of each kernel makes them meet
(tests/test_xyzz_cases.py checks on the host that they do):

  k_sum_affine        every (site, branch) of its stride loop and of block_sum's tree, through plk_curve_sum_affine and through
                      affine_multisummation_best;
  k_combine_partials  exchange records written by hand - every split of a batch into whole and sharded vectors at worlds 1 ... 8 and at
                      64, 65, 130 (a second and a third trip of the stride loop), the flag byte at every position of its 32-bit word,
                      identity, equal and opposite partials, a buffer that is used twice - and the refusals of the entry;
  k_gen_bases         G0 + (first + i) D with first + i across 2^32 and above 2^63, D = G0, D = 2 G0 and D of order 2.

Every expected value is bigint_ref's ec_add / ec_mul / ec_neg; every comparison is limb for limb after from_mont_arr, with the identity
flag.  Neither device law is compared with the other."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import plonky_amd as pa
from oracle import bigint_ref as br
from plonky_amd import api, lib as plk
from tests import xyzz_cases as xc
from tests.test_oracle_kats import from_mont_arr

CURVES = list(br.CURVES.values())


@pytest.fixture(scope="module", autouse=True)
def _device():
    from plonky_amd import device as dev
    dev.init(0)


def _same(c, xy, zero, Q):
    """affine limbs (2, L) and an identity flag against an affine big-integer point (None: the identity, whose words are zero)"""
    if Q is None:
        return int(zero) == 1 and not np.asarray(xy).any()
    return int(zero) == 0 and tuple(from_mont_arr(c.base, np.asarray(xy).reshape(2, -1))) == Q


# ---------------------------------------------------------------------------------------------
# k_sum_affine
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sums():
    """per curve: [(case, points, flags, the replay's sum)], computed once"""
    out = {}
    for c in CURVES:
        out[c.curve_id] = [(case,) + xc.sum_arrays(c, case) + (xc.schedule(c.curve_id, case.entries)[0],) for case in xc.sum_cases(c.curve_id)]
    return out


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_sum_affine_takes_every_branch(c, sums):
    wrong, identities = [], 0
    for case, xy, zero, want in sums[c.curve_id]:
        out, z = api.curve_sum_affine(c.curve_id, xy, zero)
        identities += want is None
        if not _same(c, out, z, want):
            wrong.append((case.label, case.aims, int(z)))
    for w in wrong:
        print(w)
    assert not wrong, wrong[0]
    assert identities >= 8   # zero words and flag 1: the lists that cancel, the flagged ones, the empty one


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_multisummation_takes_every_branch(c, sums):
    table = sums[c.curve_id]
    got = pa.affine_multisummation_best(c.curve_id, [xy for _, xy, _, _ in table], zeros=[zero for _, _, zero, _ in table])
    assert len(got) == len(table)
    wrong = [case.label for (case, _, _, want), (out, z) in zip(table, got) if not _same(c, out, z, want)]
    assert not wrong, wrong


# ---------------------------------------------------------------------------------------------
# k_combine_partials
# ---------------------------------------------------------------------------------------------
def _combine(c, world, batch, whole, gathered, out=None):
    """plk_msm_combine_partials_dev as parallel.PartialExchange.combine calls it; the outputs start as words no result has"""
    import torch
    from plonky_amd.device import _dp, _stream
    L = c.base.n_limbs
    if out is None:
        out = (torch.full((batch, 2, L), -1, dtype=torch.int64, device="cuda"), torch.full((batch,), 7, dtype=torch.uint8, device="cuda"))
    plk.check(plk.load().plk_msm_combine_partials_dev(c.curve_id, world, batch, whole, _dp(gathered), _dp(out[0]), _dp(out[1]), _stream()))
    torch.cuda.current_stream().synchronize()
    return out[0].cpu().numpy().view(np.uint64), out[1].cpu().numpy()


def _wrong_vectors(c, case, expected, xy, zero):
    assert xy.shape == (case.batch, 2, c.base.n_limbs) and zero.shape == (case.batch,)
    return [(case.label, v) for v, want in enumerate(expected) if want != xc.UNCHECKED and not _same(c, xy[v], zero[v], want)]


@pytest.mark.parametrize("world", xc.WORLDS)
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_combine_partials_on_handwritten_records(c, world):
    import torch
    wrong, ran = [], 0
    for case in xc.combine_cases(c.curve_id):
        if case.world != world:
            continue
        slots = xc.slots_of(case.world, case.batch, case.whole)
        assert plk.load().plk_msm_partials_bytes(c.curve_id, slots) == xc.record_bytes(c, slots)
        buf, expected = xc.combine_layout(case)
        xy, zero = _combine(c, case.world, case.batch, case.whole, torch.from_numpy(buf).cuda())
        wrong += _wrong_vectors(c, case, expected, xy, zero)
        ran += 1
    for w in wrong:
        print(w)
    assert not wrong, wrong[0]
    assert ran >= 9


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_combine_partials_follows_a_reused_buffer(c):
    """the scratch pool hands the gathered buffer out again: the second result follows the second contents"""
    import torch
    by = {case.label: case for case in xc.combine_cases(c.curve_id)}
    first, second = by["w8/hybrid-2/distinct"], by["w8/hybrid-2/checker"]
    (b1, e1), (b2, e2) = xc.combine_layout(first), xc.combine_layout(second)
    assert b1.shape == b2.shape and e1 != e2
    gathered = torch.from_numpy(b1).cuda()
    xy, zero = _combine(c, 8, first.batch, first.whole, gathered)
    assert not _wrong_vectors(c, first, e1, xy, zero)
    gathered.copy_(torch.from_numpy(b2))
    torch.cuda.current_stream().synchronize()
    xy, zero = _combine(c, 8, second.batch, second.whole, gathered)
    assert not _wrong_vectors(c, second, e2, xy, zero)


def test_combine_partials_refusals():
    import torch
    from plonky_amd.device import _dp, _stream
    L = plk.load()
    g = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    xy = torch.zeros((4, 2, 4), dtype=torch.int64, device="cuda")
    z = torch.zeros(4, dtype=torch.uint8, device="cuda")
    refused = {"world 0": (0, 0, 1, 0, _dp(g), _dp(xy), _dp(z)),
               "null gathered": (0, 1, 1, 0, None, _dp(xy), _dp(z)),
               "null out_xy": (0, 1, 1, 0, _dp(g), None, _dp(z)),
               "null out_zero": (0, 1, 1, 0, _dp(g), _dp(xy), None),
               "whole x world > batch": (0, 2, 3, 2, _dp(g), _dp(xy), _dp(z))}
    for what, args in refused.items():
        assert L.plk_msm_combine_partials_dev(*args, _stream()) == plk.PLK_ERR_INVALID_ARG, what
        assert L.plk_last_error().decode("utf-8", "replace").strip(), what
    # an empty batch is a no-op before the pointers are looked at
    assert L.plk_msm_combine_partials_dev(0, 0, 0, 0, None, None, None, _stream()) == plk.PLK_OK
    assert L.plk_msm_combine_partials_dev(0, 2, 0, 5, None, None, None, _stream()) == plk.PLK_OK
    torch.cuda.current_stream().synchronize()
    assert not xy.any() and not z.any()


# ---------------------------------------------------------------------------------------------
# k_gen_bases
# ---------------------------------------------------------------------------------------------
def _gen(c, n, G0, D, first):
    from plonky_amd import device as dev
    g0, dd = xc.points_to_arrays(c, [G0])[0][0], xc.points_to_arrays(c, [D])[0][0]
    got = dev.to_host(dev.gen_bases_dev(c.curve_id, n, g0, dd, first=first))
    assert got.shape == (n, 2, c.base.n_limbs)
    return [tuple(from_mont_arr(c.base, got[i])) for i in range(n)]


def _gen_expected(c, n, G0, D, first):
    M = br.ec_mul(c, first, D)
    out = []
    for _ in range(n):
        out.append(br.ec_add(c, G0, M))
        M = br.ec_add(c, M, D)
    return out


@pytest.mark.parametrize("first", [0, 1, (1 << 32) - 2, (1 << 63) + 5])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_gen_bases_at_every_offset(c, first):
    G = (c.gx, c.gy)
    G0, D = br.ec_mul(c, 0x1F3, G), br.ec_mul(c, 0xABCDEF, G)
    for n in (1, 127, 128, 129):
        want = _gen_expected(c, n, G0, D, first)
        assert want[-1] == br.ec_add(c, G0, br.ec_mul(c, first + n - 1, D)) and None not in want
        got = _gen(c, n, G0, D, first)
        wrong = [i for i in range(n) if got[i] != want[i]]
        assert not wrong, (n, first, wrong[:4])


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_gen_bases_with_a_step_that_meets_the_start(c):
    """D = G0: i = 0 adds G0 to an identity accumulator, i = 1 adds G0 to G0 (xyzz_mdbl); D = 2 G0: the odd multiples"""
    G0 = br.ec_mul(c, 0x1F3, (c.gx, c.gy))
    for mult in (1, 2):
        D = br.ec_mul(c, mult, G0)
        want = _gen_expected(c, 129, G0, D, 0)
        assert want[0] == G0 and want[1] == br.ec_mul(c, 1 + mult, G0) and want[128] == br.ec_mul(c, 1 + 128 * mult, G0)
        assert _gen(c, 129, G0, D, 0) == want, mult


def test_gen_bases_with_a_step_of_order_two():
    """BLS12-377, D = T = (p - 1, 0): every doubling inside the double-and-add gives the identity; G0 and G0 + T alternate"""
    c = br.BLS12_377
    Tp = (c.base.p - 1, 0)
    G0 = br.ec_mul(c, 0x1F3, (c.gx, c.gy))
    G0T = br.ec_add(c, G0, Tp)
    assert G0T not in (None, G0) and br.ec_add(c, G0T, Tp) == G0
    for first in (0, 1, (1 << 32) - 2, (1 << 63) + 5):
        want = [G0T if (first + i) & 1 else G0 for i in range(129)]
        assert want == _gen_expected(c, 129, G0, Tp, first)
        assert _gen(c, 129, G0, Tp, first) == want, first
