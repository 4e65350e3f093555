"""Inputs of the Plookup sorted multiset shared by its CPU and GPU tests (tests/test_plookup_sort_host_replay.py,
tests/test_gpu_plookup_sort.py): limb arrays f (N, 4) = f_padded (the last row is not read) and t (N, 4), rows as the reference stores
them.  The sort compares words only, so any 4 x 64 bit rows will do where no field is named."""
import numpy as np

ZERO_ROW = np.zeros((1, 4), dtype=np.uint64)


def pad_f(f_rows):
    """n rows -> f_padded (N rows): the row the device entry does not read"""
    return np.ascontiguousarray(np.concatenate([f_rows, ZERO_ROW]))


def distinct_rows(rng, count):
    """`count` distinct random rows, none of them zero (numpy Generator)"""
    while True:
        rows = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) | np.uint64(1)
        if len({r.tobytes() for r in rows}) == count:
            return rows


def drawn(rng, t, count):
    """`count` rows drawn from t with repeats, and the indices"""
    idx = rng.integers(0, t.shape[0], size=count)
    return t[idx], idx


def distinct_case(rng, log_size):
    size = 1 << log_size
    t = distinct_rows(rng, size)
    return pad_f(drawn(rng, t, size - 1)[0]), t


def duplicate_case(rng, log_size, first, second):
    """t distinct but for row `second`, a copy of row `first` < `second`; a share of f hits the value"""
    size = 1 << log_size
    assert 0 <= first < second < size
    t = distinct_rows(rng, size)
    t[second] = t[first]
    f = drawn(rng, t, size - 1)[0]
    f[:: 3] = t[second]
    return pad_f(f), t


def padded_case(rng, log_size, n_f, n_t):
    """pad_inputs (plookup.rs:155-167): n_f table values then zeros in f, n_t distinct values then zeros in t"""
    size = 1 << log_size
    t = np.zeros((size, 4), dtype=np.uint64)
    t[:n_t] = distinct_rows(rng, n_t)
    f = np.zeros((size - 1, 4), dtype=np.uint64)
    f[:n_f] = drawn(rng, t[:n_t], n_f)[0]
    return pad_f(f), t


def structured_case(rng, log_size, limb, shift=0):
    """rows [i,0,0,0] (limb 0: they differ in the lowest word only) or [0,0,0,i] (limb 3; with shift = 32 the highest word of the row),
    in a shuffled order"""
    size = 1 << log_size
    t = np.zeros((size, 4), dtype=np.uint64)
    t[:, limb] = rng.permutation(size).astype(np.uint64) << np.uint64(shift)
    return pad_f(drawn(rng, t, size - 1)[0]), t


def restatement(f, t):
    """s, the rows of f outside t and the distinct values of t from counts alone: t_i repeated c_i times for every first occurrence i"""
    first, rep = {}, np.empty(t.shape[0], dtype=np.int64)
    for i, row in enumerate(t):
        rep[i] = first.setdefault(row.tobytes(), i)
    cnt = np.bincount(rep, minlength=t.shape[0])
    missing = 0
    for row in f[:-1]:
        i = first.get(row.tobytes())
        if i is None:
            missing += 1
        else:
            cnt[i] += 1
    s = np.zeros((2 * t.shape[0] - 1, 4), dtype=np.uint64)
    s[: int(cnt.sum())] = np.repeat(t, cnt, axis=0)
    return s, missing, len(first)
