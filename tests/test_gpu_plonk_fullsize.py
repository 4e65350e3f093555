"""GPU tests of the quotient numerator (plk_plonk_vanishing_points_dev, plonk.rs:392-453) at the sizes it runs at, up to the
production size of 2^20 gates (2^23 points), on every scalar field the entry dispatches.  A full reference run is out of reach there
(hours of big-integer arithmetic, gigabytes of host tables), so each case compares a fixed boundary set and seeded random rows of the
device output, bit for bit, with the one-row big-integer restatement br.plonk_vanishing_point.

Inputs are drawn on the device, every element independently (no tiling of a smaller table), then words from extreme_words are planted
into the entries that a third of the sampled points read.  The test asserts, per case: every sampled row is compared; every boundary
row is in the sample; every row of the input conversion's top-part table (plonk.hip lz_from_rform) is read by some sampled point; no two
sampled points read the same tuple of input words (an index error that lands on another sampled point cannot go unseen); the device
inputs are unchanged after the call.
"""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from oracle import oracle_lib as ol
from tests.test_oracle_plonk import extreme_words
from tests.util import ints_to_array

TABLES = (("constants", br.NUM_CONSTANTS), ("wires", br.NUM_WIRES), ("s_sigma", br.NUM_ROUTED_WIRES), ("z", 1))
RANDOM_ROWS = 4096


def device_words(f, shape, gen):
    """int64 CUDA tensor shape + (4,) of stored words, each element independent: four uniform 64-bit limbs with the top limb masked
    below the top bit of p, so every word is canonical (< 2^(bitlen(p) - 1) < p).  Words in [2^(bitlen(p) - 1), p) come from planting."""
    import torch
    t = torch.randint(-(1 << 31), 1 << 31, tuple(shape) + (8,), dtype=torch.int32, device="cuda", generator=gen).view(torch.int64)
    t[..., 3] &= (1 << (f.p.bit_length() - 1 - 192)) - 1
    return t


def clear_device_caches():
    import torch
    from plonky_amd import lib
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    lib.check(lib.load().plk_ntt_clear_cache())  # also drops the cached circuit-size tables (powers of the root, L_1)


def boundary_rows(log_n8):
    """Where the indexing changes: the first rows, the low / high power-table split at 2^10, every power of two (the high table's
    index bits), the middle, the wrap-around of the right (+8) and below (+8 * 65) neighbours, the last rows."""
    n8 = 1 << log_n8
    rows = {0, 1, 7, 8, 9, 127, 128, 1023, 1024, 1025, n8 // 2 - 1, n8 // 2, n8 - 521, n8 - 520, n8 - 519, n8 - 9, n8 - 8, n8 - 7, n8 - 1}
    for k in range(11, log_n8):
        rows |= {(1 << k) - 1, 1 << k}
    return sorted(rows)


def top_row(f, word):
    """Row of the top-part table (plonk.hip LzSplit) that the input conversion reads for a stored word."""
    return word >> (f.p.bit_length() - 1 - 5)


# (field, log_degree, challenges): the size ladder on TweedledumBase, every other dispatch at 2^20 points, edge challenges
CASES = [
    (br.TWEEDLEDUM_BASE, 14, "random"),
    (br.TWEEDLEDUM_BASE, 17, "random"),
    (br.TWEEDLEDUM_BASE, 20, "random"),
    (br.TWEEDLEDEE_BASE, 17, "random"),
    (br.BLS12_377_SCALAR, 17, "random"),
    (br.PALLAS_BASE, 17, "random"),
    (br.VESTA_BASE, 17, "random"),
    (br.TWEEDLEDUM_BASE, 17, "edge"),
]


@pytest.mark.parametrize("f,log_degree,challenges", CASES, ids=["%s-d%d-%s" % (f.name, d, c) for f, d, c in CASES])
def test_vanishing_points_sampled_rows(f, log_degree, challenges):
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    degree = 1 << log_degree
    log_n8 = log_degree + 3
    n8 = 1 << log_n8
    seed = 0xF0115 + 64 * log_degree + 8 * f.field_id + (challenges == "edge")
    rng = random.Random(seed)
    ext = extreme_words(f)
    ext_arr = ints_to_array(ext, 4).view(np.int64)

    # challenges and shifts: canonical words
    if challenges == "random":
        sc = ol.rand_field(f.field_id, seed, 11)
        k_is, (alpha, beta, gamma, zeta, a) = sc[:6], sc[6:]
    else:
        word = lambda v: ints_to_array([v], 4)[0]
        alpha, beta, gamma, zeta, a = word(f.p - 1), word(f.p - 2), word(0), word(f.p - 1), word(f.p - 1)
        k_is = ints_to_array([rng.choice(ext) for _ in range(6)], 4)

    # the sample: the boundary set and seeded random rows
    boundary = boundary_rows(log_n8)
    sample = sorted(set(boundary) | set(rng.sample(range(n8), RANDOM_ROWS)))
    reads = {i: br.plonk_vanishing_point_reads(degree, i) for i in sample}

    # planting: at a third of the sampled points, the point's own selector constants, sigma values, Z value and two of its wires.  A point
    # reads at most 6 + 6 + 1 + 2 of its own, 2 + 1 of its right neighbour's and 2 of the one below it: 20 of its 41 inputs
    planted_points = rng.sample(sample, (len(sample) + 2) // 3)
    planted = {name: [] for name, _ in TABLES}
    for i in planted_points:
        planted["constants"] += [(j, i) for j in range(br.NUM_CONSTANTS)]
        planted["s_sigma"] += [(j, i) for j in range(br.NUM_ROUTED_WIRES)]
        planted["z"].append((0, i))
        planted["wires"] += [(j, i) for j in rng.sample(range(br.NUM_WIRES), 2)]
    planted_set = {(name, j, i) for name, pos in planted.items() for j, i in pos}

    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    tabs, copies, out = {}, {}, None
    try:
        for name, rows in TABLES:
            t = device_words(f, (rows, n8), gen)
            pos = planted[name]
            rj = torch.tensor([p[0] for p in pos], dtype=torch.int64, device="cuda")
            ri = torch.tensor([p[1] for p in pos], dtype=torch.int64, device="cuda")
            t[rj, ri] = torch.from_numpy(ext_arr[[rng.randrange(len(ext)) for _ in pos]]).to("cuda")
            tabs[name] = t
            copies[name] = t.clone()
        out = dev.vanishing_points_dev(f.field_id, log_degree, tabs["constants"], tabs["wires"], tabs["s_sigma"], tabs["z"][0], k_is, alpha, beta,
                                       gamma, zeta, a)
        torch.cuda.synchronize()
        # (e) the inputs are unchanged
        changed = [name for name, _ in TABLES if not torch.equal(tabs[name], copies[name])]
        # the entries the reference needs, copied back from the tensors the kernel read, and the sampled outputs
        cols = sorted({idx for i in sample for _, _, idx in reads[i]})
        col_t = torch.tensor(cols, dtype=torch.int64, device="cuda")
        host = {name: dev.to_host(tabs[name][:, col_t]) for name, _ in TABLES}
        got = dev.to_host(out[torch.tensor(sample, dtype=torch.int64, device="cuda")])
    finally:
        tabs = copies = out = None
        clear_device_caches()
    assert not changed, "device inputs modified: %s" % changed

    at = {idx: c for c, idx in enumerate(cols)}
    word_of = lambda name, j, idx: br.limbs_to_int(host[name][j, at[idx]])
    canon = {}

    def value(name, j, idx):
        key = (name, j, idx)
        if key not in canon:
            canon[key] = f.from_mont(word_of(name, j, idx))
        return canon[key]

    # (b) every boundary row is sampled
    assert set(boundary) <= set(sample)
    # planting: a quarter of the sampled points or more read a planted word, none reads more than half planted words
    hits = [sum(r in planted_set for r in reads[i]) for i in sample]
    assert sum(h > 0 for h in hits) * 4 >= len(sample), sum(h > 0 for h in hits)
    assert max(hits) * 2 <= len(reads[sample[0]]), max(hits)
    # (c) every row of the top-part table is read by a sampled point
    tmax = (f.p - 1) >> (f.p.bit_length() - 1 - 5)
    seen = {top_row(f, word_of(*r)) for i in sample for r in reads[i]}
    assert seen == set(range(tmax + 1)), sorted(set(range(tmax + 1)) - seen)
    # (d) no two sampled points read the same tuple of input words
    tuples = {b"".join(host[name][j, at[idx]].tobytes() for name, j, idx in reads[i]) for i in sample}
    assert len(tuples) == len(sample)

    one = lambda v: f.from_mont(br.limbs_to_int(v))
    scal = ([one(k_is[j]) for j in range(6)], one(alpha), one(beta), one(gamma), one(zeta), one(a))
    exp = br.plonk_vanishing_points_at(f, degree, sample, lambda j, i: value("constants", j, i), lambda j, i: value("wires", j, i),
                                       lambda j, i: value("s_sigma", j, i), lambda i: value("z", 0, i), *scal)
    compared, bad = 0, []
    for row, g, e in zip(sample, got, exp):
        compared += 1
        if br.limbs_to_int(g) != f.to_mont(e):
            bad.append(row)
    # (a) no sampled row is left out
    assert compared == len(sample) == len(exp)
    assert not bad, "%d of %d sampled rows differ, first %s" % (len(bad), compared, bad[:8])
