"""Inputs of the sigma tests (tests/test_sigma_host_replay.py on the host, tests/test_gpu_sigma.py on the device): wire partitions in
the flattened form of plk_plonk_sigma[_dev] - members (wire ids input * n + gate) and offsets - and the numpy restatement of the
neighbour rule both compare with.  Everything is seeded; nothing here calls the library."""
import numpy as np

from tests import partition_ref as pref

ROUTED, WIRES = pref.NUM_ROUTED_WIRES, pref.NUM_WIRES


def csr(parts):
    """list of lists of wire ids -> (members, offsets) uint32"""
    offsets = np.zeros(len(parts) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(p) for p in parts])
    members = np.array([m for p in parts for m in p], dtype=np.uint32)
    return members, offsets


def neighbour_rule(members, offsets, n):
    """sigma by the rule of the issue, restated with numpy: the member after slot p in its partition, the first after the last;
    sigma[members[p]] for the routed members.  Entries no slot writes stay 0xFFFFFFFF."""
    members, offsets = np.asarray(members, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
    sizes = np.diff(offsets)
    begin, end = np.repeat(offsets[:-1], sizes), np.repeat(offsets[1:], sizes)
    p = np.arange(members.shape[0], dtype=np.int64)
    nb = np.where(p + 1 < end, p + 1, begin)
    sigma = np.full(ROUTED * n, 0xFFFFFFFF, dtype=np.uint32)
    routed = members < ROUTED * n
    sigma[members[routed]] = members[nb[routed]]
    return sigma


def singletons(n, list_non_routed=True):
    return csr([[w] for w in range((WIRES if list_non_routed else ROUTED) * n)])


def one_cycle(n, seed):
    """one partition that holds all 6n routed wires in a seeded order: neighbours cross columns, the last slot wraps to slot 0"""
    order = np.random.default_rng(seed).permutation(ROUTED * n)
    return csr([order.tolist()])


def pair_partitions(n, seed):
    """the 6n routed wires in 3n seeded pairs"""
    order = np.random.default_rng(seed).permutation(ROUTED * n).tolist()
    return [order[i:i + 2] for i in range(0, len(order), 2)]


def listing_variants(n, seed):
    """the same pairs listed in six ways: pairs only; with the non-routed wires as singletons behind, in front and in between; with
    empty partitions at the front, at the back and between two others; with a run of 600 empty partitions in the middle (a workgroup
    whose slots span more partitions than its copy of the offsets holds).  All have the same sigma."""
    pairs = pair_partitions(n, seed)
    non_routed = [[w] for w in range(ROUTED * n, WIRES * n)]
    half = len(pairs) // 2
    mixed = []
    for k, pr in enumerate(pairs):
        mixed.append(pr)
        if k < len(non_routed):
            mixed.append(non_routed[k])
    mixed += non_routed[len(pairs):]
    return {
        "pairs only": csr(pairs),
        "non-routed behind": csr(pairs + non_routed),
        "non-routed in front": csr(non_routed + pairs),
        "non-routed in between": csr(mixed),
        "empty partitions": csr([[], [], []] + pairs[:half] + [[]] + pairs[half:half + 1] + [[], []] + pairs[half + 1:] + [[], []]),
        "a run of empty partitions": csr(pairs[:half] + [[]] * 600 + pairs[half:]),
    }


SEAM_SIZES = (255, 256, 257, 511, 1025)


def seams(n, seed):
    """partitions of 255, 256, 257, 511 and 1025 members packed back to back, again and again until the 6n routed wires are used up
    (the last one takes what is left): wrap-arounds on either side of the edges of 256-slot workgroups"""
    order = np.random.default_rng(seed).permutation(ROUTED * n).tolist()
    parts, pos, k = [], 0, 0
    while pos < len(order):
        size = min(SEAM_SIZES[k % len(SEAM_SIZES)], len(order) - pos)
        parts.append(order[pos:pos + size])
        pos += size
        k += 1
    return csr(parts)


def skew(n, seed):
    """one partition of n / 2 routed wires scattered over the columns by a seeded permutation, every other wire a singleton"""
    order = np.random.default_rng(seed).permutation(ROUTED * n)
    big = order[: n // 2]
    rest = np.sort(order[n // 2:])
    members = np.concatenate([rest[: rest.shape[0] // 2], big, rest[rest.shape[0] // 2:]]).astype(np.uint32)
    a = rest.shape[0] // 2
    offsets = np.concatenate([np.arange(a + 1), a + big.shape[0] + np.arange(rest.shape[0] - a + 1)]).astype(np.uint32)
    return members, offsets


def merge_sequence(n, seed, n_virtual, n_merges, cap=None):
    """a seeded sequence of merges over the routed wires of n gates and n_virtual virtual targets, as a list of (a, b) targets.  It
    holds repeated merges of one pair, merges into an already merged class from either side and virtual targets that bridge wires;
    every merge leaves a stale list behind.  cap: merges that would make a class larger than cap are left out (sizes are followed
    with a union-find of this function's own)."""
    rng = np.random.default_rng(seed)
    targets = [("wire", g, i) for g in range(n) for i in range(ROUTED)] + [("virtual", v) for v in range(n_virtual)]
    parent = list(range(len(targets)))
    size = [1] * len(targets)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    ops = []
    picks = rng.integers(0, len(targets), size=(n_merges, 2))
    for k, (a, b) in enumerate(picks.tolist()):
        if k % 7 == 3 and ops:
            a, b = ops[-1][1], ops[-1][0]          # the same pair again, the other way round
        elif k % 7 == 5 and ops:
            a = ops[int(rng.integers(0, len(ops)))][0]  # a member of a class merged earlier, on the a side
        elif k % 7 == 6 and ops:
            b = ops[int(rng.integers(0, len(ops)))][1]  # ... on the b side
        ra, rb = find(a), find(b)
        if ra != rb:
            if cap is not None and size[ra] + size[rb] > cap:
                continue
            parent[ra] = rb
            size[rb] += size[ra]
        ops.append((a, b))
    return [(targets[a], targets[b]) for a, b in ops]


def build_partitions(cls, n, ops, n_virtual):
    """a TargetPartitions (the mirror or the restatement) with every wire of n gates and the virtual targets, then the merges"""
    tp = cls()
    for g in range(n):
        for i in range(WIRES):
            tp.add_partition(("wire", g, i))
    for v in range(n_virtual):
        tp.add_partition(("virtual", v))
    for a, b in ops:
        tp.merge(a, b)
    return tp


def bad_cases(n, seed):
    """name -> (members, offsets, status words): one defect each, on the pairs of listing_variants"""
    pairs = pair_partitions(n, seed)
    non_routed = [[w] for w in range(ROUTED * n, WIRES * n)]
    twice = [list(p) for p in pairs] + [[pairs[0][0]]]
    missing = [list(p) for p in pairs[:-1]] + [[pairs[-1][0]]]
    lonely = [list(p) for p in pairs[:-1]] + [[pairs[-1][0]], [pairs[-1][1], ROUTED * n + 1]]
    return {
        "one wire listed twice": csr(twice) + ([1, 0, 0],),
        "one wire left out": csr(missing) + ([1, 0, 0],),
        "a non-routed wire in a pair": csr(lonely) + ([0, 1, 0],),
        "valid": csr(pairs + non_routed) + ([0, 0, 0],),
    }


def out_of_range_case(n, seed):
    """id = 9n among the singletons (host replay only: no out-of-range id goes to the GPU)"""
    members, offsets = singletons(n)
    members = np.concatenate([members, np.array([WIRES * n], dtype=np.uint32)])
    offsets = np.concatenate([offsets, np.array([members.shape[0]], dtype=np.uint32)])
    return members, offsets, [0, 0, 1]
