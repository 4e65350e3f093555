"""GPU tests of the Plookup sorted multiset on the device (plk_plookup_sorted_multiset[_dev], plookup_sort.hip): word-for-word parity
with the host helper api.plookup_sorted_multiset (and tests/plookup_ref.sort_by at <= 64 rows) on the five 4-limb fields, the padded
shapes of pad_inputs, duplicates in t, structured rows, rows of f outside t, streams and determinism, the prover's chain with s never
on the host, the refusals, and the small set through the checked build.

Sizes: the count scan gives a workgroup a tile of PSORT_TILE = PSORT_LANES x PSORT_ROWS = 256 x 4 = 1024 counts
(plookup_sort_step.cuh), so besides the small sizes 1, 2, 3, 6: log_size 10 is one tile exactly, 11 two tiles (the tile scan and the
offsets' tile prefix do work), 16 is 64 tiles.  The tile scan takes PSORT_CHUNK = 256 tile sums per step, 2^18 rows: log_size 19 is
the smallest size at which its carry between steps does work, and one case runs there."""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bigint_ref as br
from plonky_amd import api
from plonky_amd import lib as plk
from tests import checked_child
from tests import plookup_ref as pr
from tests import plookup_sort_cases as sc
from tests.test_oracle_plonk import mont, unmont

FIELDS = [br.TWEEDLEDEE_BASE, br.TWEEDLEDUM_BASE, br.BLS12_377_SCALAR, br.PALLAS_BASE, br.VESTA_BASE]
ONE_TILE, TWO_TILES, MANY_TILES, TWO_CHUNKS = 10, 11, 16, 19
F0 = br.TWEEDLEDEE_BASE.field_id
UNWRAP = "called `Option::unwrap()` on a `None` value"


def run_dev(field, log_size, f, t, stream=None):
    """-> (s, status) through the device entry; f and t are checked to be unchanged on the device afterwards"""
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    fd, td = dev.to_device(f), dev.to_device(t)
    if stream is None:
        s, st = dev.plookup_sorted_multiset_dev(field, log_size, fd, td, status=True)
    else:
        with torch.cuda.stream(stream):
            fd, td = dev.to_device(f), dev.to_device(t)
            s, st = dev.plookup_sorted_multiset_dev(field, log_size, fd, td, status=True)
        stream.synchronize()
    out = dev.to_host(s), [int(v) for v in st.cpu().tolist()]
    assert np.array_equal(dev.to_host(fd), f) and np.array_equal(dev.to_host(td), t), "inputs modified"
    return out


def field_case(f, log_size, seed):
    """t distinct field elements in the stored form, f drawn from t"""
    rng = random.Random(seed)
    size = 1 << log_size
    tv = set()
    while len(tv) < size:
        tv.add(rng.randrange(f.p))
    tv = list(tv)
    rng.shuffle(tv)
    t = mont(f, tv)
    return sc.pad_f(t[[rng.randrange(size) for _ in range(size - 1)]]), t


@pytest.mark.parametrize("log_size", [1, 2, 3, 6, ONE_TILE, TWO_TILES, MANY_TILES])
@pytest.mark.parametrize("f", FIELDS, ids=lambda f: f.name)
def test_distinct_table_on_every_field(f, log_size):
    fm, tm = field_case(f, log_size, 0x5027 + 31 * log_size + f.field_id)
    exp = api.plookup_sorted_multiset(fm[:-1], tm)
    if log_size <= 6:
        fv, tv = unmont(f, fm[:-1]), unmont(f, tm)
        assert unmont(f, exp) == pr.sort_by(fv + tv, tv)
    got, status = run_dev(f.field_id, log_size, fm, tm)
    assert status == [0, 1 << log_size]
    assert np.array_equal(got, exp)
    assert np.array_equal(api.plookup_sorted_multiset_device(f.field_id, fm, tm), exp)
    assert np.array_equal(api.plookup_sorted_multiset_device(f.field_id, fm[:-1], tm), exp), "f with n rows is padded"


def padded_shapes():
    rng = np.random.default_rng(0x9AD)
    log_size, size = MANY_TILES, 1 << MANY_TILES
    yield "f: 1000 values then zeros", sc.padded_case(rng, log_size, 1000, size - 1)
    yield "t: 3000 values then zeros", sc.padded_case(rng, log_size, size // 2, 3000)
    f, t = sc.padded_case(rng, log_size, 0, 3 * size // 4)
    f[:-1] = t[-1]
    yield "all of f equal to t's last row", (f, t)
    f, t = sc.distinct_case(rng, log_size)
    f[:-1] = t[0]
    yield "f holds only the value of row 0", (f, t)


PADDED = dict(padded_shapes())


@pytest.mark.parametrize("shape", sorted(PADDED))
def test_padded_shapes(shape):
    f, t = PADDED[shape]
    exp, missing, distinct = sc.restatement(f, t)
    assert missing == 0 and np.array_equal(exp, api.plookup_sorted_multiset(f[:-1], t))
    got, status = run_dev(F0, MANY_TILES, f, t)
    assert status == [0, distinct]
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("log_size", [6, TWO_TILES])
@pytest.mark.parametrize("where", ["early", "late"])
def test_duplicate_in_t_sorts_at_its_first_occurrence(where, log_size):
    size = 1 << log_size
    first, second = (1, size - 3) if where == "early" else (size - 3, size - 1)
    f, t = sc.duplicate_case(np.random.default_rng(0xD0B + log_size), log_size, first, second)
    exp = api.plookup_sorted_multiset(f[:-1], t)
    got, status = run_dev(F0, log_size, f, t)
    assert status == [0, size - 1] and np.array_equal(got, exp)
    # rank of the value in s: the rows before it are the rows of smaller first occurrence, each once for t and once per hit in f
    where_v = np.flatnonzero((got == t[first]).all(axis=1))
    hits = int((f[:-1] == t[first]).all(axis=1).sum())
    assert hits > 0 and len(where_v) == hits + 2 and where_v[-1] - where_v[0] == hits + 1, "the value's rows are one run"
    before = int(sum((f[:-1] == t[i]).all(axis=1).sum() for i in range(first))) + first
    assert where_v[0] == before, "the run starts at the FIRST occurrence's rank"


@pytest.mark.parametrize("limb,shift", [(0, 0), (3, 0), (3, 32)], ids=["lowest-word", "highest-limb", "highest-word"])
def test_structured_rows(limb, shift):
    log_size = 12
    f, t = sc.structured_case(np.random.default_rng(0x57 + limb + shift), log_size, limb, shift)
    got, status = run_dev(F0, log_size, f, t)
    assert status == [0, 1 << log_size] and np.array_equal(got, api.plookup_sorted_multiset(f[:-1], t))


@pytest.mark.parametrize("log_size,count", [(6, 1), (TWO_TILES, 1), (TWO_TILES, 7), (TWO_TILES, (1 << TWO_TILES) - 1), (MANY_TILES, (1 << MANY_TILES) - 1)])
def test_rows_of_f_outside_t(log_size, count):
    rng = np.random.default_rng(0x0575 + log_size + count)
    size = 1 << log_size
    n = size - 1
    f, t = sc.distinct_case(rng, log_size)
    outside = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) & ~np.uint64(1)  # the rows of t are odd in every limb
    f[rng.choice(n, size=count, replace=False)] = outside
    exp, missing, distinct = sc.restatement(f, t)
    assert missing == count and distinct == size
    got, status = run_dev(F0, log_size, f, t)
    assert status == [count, size]
    assert np.array_equal(got, exp) and not got[2 * size - 1 - count:].any(), "the tail of s is zero"
    # the host entry: the reference's panic text, *missing set, s untouched
    L = plk.load()
    s_host = np.full((2 * size - 1, 4), 0xAB, dtype=np.uint64)
    miss = ctypes.c_uint(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = L.plk_plookup_sorted_multiset(log_size, F0, p(f), p(t), p(s_host), ctypes.byref(miss))
    assert rc == plk.PLK_ERR_INVALID_ARG and L.plk_last_error().decode().startswith(UNWRAP) and miss.value == count
    assert (s_host == 0xAB).all()
    with pytest.raises(AssertionError, match="unwrap"):
        api.plookup_sorted_multiset_device(F0, f, t)
    with pytest.raises(AssertionError):
        api.plookup_sorted_multiset(f[:-1], t)


def test_side_stream_determinism_and_inputs():
    import torch
    f, t = sc.padded_case(np.random.default_rng(0x57EA), MANY_TILES, 20000, 40000)
    a, status_a = run_dev(F0, MANY_TILES, f, t)
    b, status_b = run_dev(F0, MANY_TILES, f, t)
    c, status_c = run_dev(F0, MANY_TILES, f, t, stream=torch.cuda.Stream())
    assert a.tobytes() == b.tobytes() == c.tobytes() and status_a == status_b == status_c == [0, 40001]
    assert np.array_equal(a, api.plookup_sorted_multiset(f[:-1], t))


def test_status_is_optional_and_out_is_used():
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    f, t = sc.distinct_case(np.random.default_rng(0x0B7), TWO_TILES)
    out = torch.zeros(((2 << TWO_TILES) - 1, 4), dtype=torch.int64, device="cuda")
    got = dev.plookup_sorted_multiset_dev(F0, TWO_TILES, dev.to_device(f), dev.to_device(t), out=out)
    assert got is out and np.array_equal(dev.to_host(out), api.plookup_sorted_multiset(f[:-1], t))


def test_tile_scan_carries_between_steps():
    """2^19 rows: 512 tile sums, two steps of the single-workgroup tile scan.  The expected s comes from the drawn indices alone."""
    log_size, size = TWO_CHUNKS, 1 << TWO_CHUNKS
    rng = np.random.default_rng(0xC4A7)
    t = sc.distinct_rows(rng, size)
    f_rows, idx = sc.drawn(rng, t, size - 1)
    got, status = run_dev(F0, log_size, sc.pad_f(f_rows), t)
    assert status == [0, size]
    assert np.array_equal(got, np.repeat(t, np.bincount(idx, minlength=size) + 1, axis=0))


def test_chain_sort_then_grand_product_stays_on_the_device():
    """honest f and t on the device: the sort, then the grand product on the SAME device tensor; the argument closes"""
    from plonky_amd import device as dev
    dev.init(0)
    f, log_size = br.TWEEDLEDUM_BASE, 12
    fm, tm = field_case(f, log_size, 0xC4A1)
    rng = random.Random(0xC4A2)
    beta, gamma = (mont(f, [rng.randrange(f.p)])[0] for _ in range(2))
    fd, td = dev.to_device(fm), dev.to_device(tm)
    sd, st_sort = dev.plookup_sorted_multiset_dev(f.field_id, log_size, fd, td, status=True)
    z, st = dev.plookup_grand_polynomial_dev(f.field_id, log_size, fd, td, sd, beta, gamma, status=True)
    assert st.cpu().tolist() == [0, 1], "the grand product over the device's s closes"
    assert st_sort.cpu().tolist() == [0, 1 << log_size]
    s_host = api.plookup_sorted_multiset(fm[:-1], tm)
    assert np.array_equal(dev.to_host(sd), s_host)
    assert np.array_equal(dev.to_host(z), api.plookup_grand_polynomial(f.field_id, fm, tm, s_host, beta, gamma))
    zi = unmont(f, dev.to_host(z))
    assert zi[0] == 1 and zi[-1] == 1 and len(set(zi)) > len(zi) // 2, "Z is not constant"


P, S = "P", "S"
CALLS = {"plk_plookup_sorted_multiset_dev": (P, P, P, P, S), "plk_plookup_sorted_multiset": (P, P, P, P)}  # after (log_size, field)


@pytest.fixture(scope="module")
def pinned():
    """64 KiB of pinned memory that host and device can both address, with a pattern no refused call may disturb"""
    import torch
    from plonky_amd import device as dev
    dev.init(0)
    return torch.full((8192,), 0x5A5A, dtype=torch.int64).pin_memory()


@pytest.mark.parametrize("name", sorted(CALLS))
def test_refused_arguments(pinned, name):
    L = plk.load()
    fn = getattr(L, name)
    args = [pinned.data_ptr() if a == P else None for a in CALLS[name]]
    for log_size, field in [(2, -1), (2, 6), (2, 1000), (2, 3), (0, 0), (29, 0), (0, 3)]:
        rc = fn(log_size, field, *args)
        err = L.plk_last_error().decode("utf-8", "replace")
        assert rc == plk.PLK_ERR_INVALID_ARG, (name, log_size, field, rc, err)
        assert ("bad field id %d" % field in err) if log_size == 2 else ("log_size %d" % log_size in err), (name, err)
    import torch
    torch.cuda.synchronize()
    assert bool((pinned == 0x5A5A).all()), "a refused call wrote"


def run_small_set():
    """a reduced set for the checked build (log_size <= 10): distinct tables on two fields, the padded shape, duplicates, a missing row"""
    compared = 0
    rng = np.random.default_rng(0xC4EC)
    for f in (br.TWEEDLEDEE_BASE, br.BLS12_377_SCALAR):
        for log_size in (1, 3, ONE_TILE):
            fm, tm = field_case(f, log_size, 0xC4ED + log_size)
            got, status = run_dev(f.field_id, log_size, fm, tm)
            assert status == [0, 1 << log_size] and np.array_equal(got, api.plookup_sorted_multiset(fm[:-1], tm))
            compared += 1
    cases = [sc.padded_case(rng, ONE_TILE, 300, 700), sc.padded_case(rng, 6, 10, 20), sc.duplicate_case(rng, ONE_TILE, 1, 1000),
             sc.duplicate_case(rng, ONE_TILE, 1020, 1023), sc.structured_case(rng, ONE_TILE, 0)]
    f, t = sc.distinct_case(rng, ONE_TILE)
    f[5] = 0
    cases.append((f, t))
    for f, t in cases:
        exp, missing, distinct = sc.restatement(f, t)
        got, status = run_dev(F0, int(np.log2(t.shape[0])), f, t)
        assert status == [missing, distinct] and np.array_equal(got, exp)
        compared += 1
    return compared


CHECKED_BODY = '''
from tests.test_gpu_plookup_sort import run_small_set
print("CHECKED compared", run_small_set())
'''


def test_checked_build_runs_the_small_set():
    assert "CHECKED compared 12" in checked_child.run_checked(CHECKED_BODY)
