"""The case table of the structured-input NTT tests (tests/test_ntt_structured_cases.py checks it on the host,
tests/test_gpu_ntt_structured.py runs it through k_ntt_pass): input vectors a real witness is made of - zeros, ones, constants, sparse
columns - and, where one exists, the closed form of their transform as Python integers.

For a field f, n = 2^log_n and w = f.primitive_root_of_unity(log_n) the forward transform is out[j] = sum_k x_k w^(jk) (fft.rs:103-156)
and the inverse is the forward one read at -j, times n^-1 (fft.rs:82-101):

  zero             all 0                                  -> all 0
  delta(i, v)      v at i, 0 elsewhere                    -> v w^(ij)             inverse  v w^(-ij) / n
  constant(c)      every entry c                          -> n c at 0, 0 elsewhere          c at 0
  geometric(m, c)  x_k = c w^(-mk)                        -> n c at m, 0 elsewhere          c at (n - m) mod n
  alternating      (1, p - 1, 1, p - 1, ..)               no closed form here: bigint_ref.ntt / the oracle
  half_zero_tail   seeded values, then n / 2 zeros        likewise
  half_zero_head   n / 2 zeros, then seeded values        likewise

constant(c) is geometric(0, c) and alternating is geometric(n / 2, 1) for n >= 2; alternating is kept apart so that one case is built
from the literal values alone.  delta(0, p - 1) puts -1 into every butterfly of every stage: a - w b + 2p with a = b up to a multiple of
p.  The exact zeros of constant and geometric are differences of equal operands at every stage.

Raw-word patterns are elements whose MONTGOMERY words - the array a caller hands in - are chosen, not their values: all ones below the
top bit, the neighbours of every 29-bit limb boundary of the kernel's working form, p - 1, p - 2.  They come as one vector cycling through
all of them, a constant vector per pattern (the closed form above with c = f.from_mont(words)) and delta(0, pattern).

Vectors of n distinct powers of w are gathered from one table of Montgomery words per (field, log_n); the host test rebuilds each of
them value by value.  Everything is seeded and plain Python / numpy; nothing here calls the library or the oracle."""
import functools
from collections import namedtuple

import numpy as np

from oracle import bigint_ref as br
from plonky_amd import synth
from tests.test_oracle_kats import mont_arr
from tests.util import ints_to_array

LIMB_BITS = 29   # the limbs of the kernel's working form (fz.cuh)

# name; x: (n, L) uint64 Montgomery words; values: () -> the n canonical values of x; fwd / inv: () -> the closed form of the forward /
# inverse transform as n canonical integers, or None where the table gives none
Case = namedtuple("Case", "name x values fwd inv")


def raw_patterns(f):
    """[(name, words)]: the chosen Montgomery words as integers, every one below p."""
    p, b = f.p, f.p.bit_length()
    out = [("p-1", p - 1), ("p-2", p - 2), ("(p-1)/2", (p - 1) // 2), ("2^(b-1)-1", (1 << (b - 1)) - 1)]
    bounds = [j for j in range(1, (b + LIMB_BITS - 1) // LIMB_BITS) if (1 << (LIMB_BITS * j)) < p]
    out += [("2^%d" % (LIMB_BITS * j), 1 << (LIMB_BITS * j)) for j in bounds]
    out += [("2^%d-1" % (LIMB_BITS * j), (1 << (LIMB_BITS * j)) - 1) for j in bounds]
    alt = sum(((1 << LIMB_BITS) - 1) << (LIMB_BITS * j) for j in range(1, (b + LIMB_BITS - 1) // LIMB_BITS, 2))
    out += [("alt-limbs", alt & ((1 << (b - 1)) - 1)), ("1", 1), ("0", 0)]
    return out


@functools.lru_cache(maxsize=None)
def _powers(field_id, log_n):
    """(w^k for k < n as canonical integers, the same as an (n, L) array of Montgomery words)"""
    f = br.FIELDS[field_id]
    w, p = f.primitive_root_of_unity(log_n), f.p
    pw = [1] * (1 << log_n)
    for k in range(1, 1 << log_n):
        pw[k] = pw[k - 1] * w % p
    return pw, mont_arr(f, pw)


def _one_hot(f, n, at, v):
    out = [0] * n
    out[at] = v % f.p
    return out


def _delta(f, log_n, i, v, words=None, name=None):
    """v at i; `words`: the element's Montgomery words instead (v is then their value)"""
    n, p = 1 << log_n, f.p
    pw = _powers(f.field_id, log_n)[0]
    x = np.zeros((n, f.n_limbs), dtype=np.uint64)
    x[i] = ints_to_array([words], f.n_limbs)[0] if words is not None else mont_arr(f, [v])[0]
    v_n = v * pow(n, -1, p) % p
    return Case(name or "delta(%s,%s)" % (_index_name(i, n), "1" if v == 1 else "p-1"), x, lambda: _one_hot(f, n, i, v),
                lambda: [v * pw[i * j % n] % p for j in range(n)] if i else [v % p] * n,
                lambda: [v_n * pw[-i * j % n] % p for j in range(n)] if i else [v_n] * n)


def _geometric(f, log_n, m, c, name):
    """x_k = c w^(-mk), c in {1, p - 1}: gathered from the power table, -w^e = w^(e + n/2)"""
    n, p = 1 << log_n, f.p
    pw, pw_words = _powers(f.field_id, log_n)
    assert c == 1 or (c == p - 1 and n >= 2)
    shift = 0 if c == 1 else n // 2
    idx = [(-m * k + shift) % n for k in range(n)]
    return Case(name, pw_words[idx], lambda: [pw[e] for e in idx], lambda: _one_hot(f, n, m, n * c), lambda: _one_hot(f, n, -m % n, c))


def _constant(f, log_n, c, words=None, name=None):
    n = 1 << log_n
    row = ints_to_array([words], f.n_limbs) if words is not None else mont_arr(f, [c])
    return Case(name or "constant(%s)" % ("1" if c == 1 else "p-1"), np.repeat(row, n, axis=0), lambda: [c % f.p] * n,
                lambda: _one_hot(f, n, 0, n * c), lambda: _one_hot(f, n, 0, c))


def _index_name(i, n):
    return {0: "0", 1: "1", n // 2: "n/2", n - 1: "n-1"}.get(i, str(i)) if n > 2 else str(i)


def _from_words(f, name, x):
    return Case(name, x, lambda: [f.from_mont(v) for v in _ints(x)], None, None)


def _ints(x):
    return [br.limbs_to_int(r) for r in x]


def pattern_cycle(f, n):
    """(n, L): the raw-word patterns of f, one after the other, again and again"""
    pats = ints_to_array([w for _, w in raw_patterns(f)], f.n_limbs)
    return pats[np.arange(n) % pats.shape[0]]


def random_vector(f, log_n, salt=0):
    return synth.rand_field(f.field_id, 0x57C000 + 64 * salt + log_n, 1 << log_n)


@functools.lru_cache(maxsize=2)
def cases(field_id, log_n):
    """Every case of the table for one field and size, in a fixed order; names are unique."""
    f = br.FIELDS[field_id]
    n, p = 1 << log_n, f.p
    out = [Case("zero", np.zeros((n, f.n_limbs), dtype=np.uint64), lambda: [0] * n, lambda: [0] * n, lambda: [0] * n)]
    for i in sorted({0, 1, n // 2, n - 1}):
        for v in (1, p - 1):
            out.append(_delta(f, log_n, i, v))
    for c in (1, p - 1):
        out.append(_constant(f, log_n, c))
    for m in sorted({1, n // 2, n - 1}):
        for c in (1, p - 1):
            out.append(_geometric(f, log_n, m, c, "geometric(%s,%s)" % (_index_name(m, n), "1" if c == 1 else "p-1")))
    one, neg = mont_arr(f, [1, p - 1])
    alt = np.empty((n, f.n_limbs), dtype=np.uint64)
    alt[0::2], alt[1::2] = one, neg
    out.append(_from_words(f, "alternating", alt))
    r = random_vector(f, log_n)
    tail, head = r.copy(), r.copy()
    tail[n // 2:] = 0
    head[: n // 2] = 0
    out.append(_from_words(f, "half_zero_tail", tail))
    out.append(_from_words(f, "half_zero_head", head))
    out.append(_from_words(f, "raw_cycle", pattern_cycle(f, n)))
    for name, words in raw_patterns(f):
        c = f.from_mont(words)
        out.append(_constant(f, log_n, c, words=words, name="raw_constant(%s)" % name))
        out.append(_delta(f, log_n, 0, c, words=words, name="raw_delta(0,%s)" % name))
    assert len({c.name for c in out}) == len(out)
    return out


def case(field_id, log_n, name):
    return next(c for c in cases(field_id, log_n) if c.name == name)


# ---- zero padding: fft_with_precomputation (fft.rs:60-80) takes any length up to n ----
def padded_lengths(log_n, first_pass_log):
    """The input lengths that visit every number of skipped stages of a first pass of 2^first_pass_log rows, on both sides of each
    threshold: the run of plan stages skips k stages when in_len <= n >> k (and not n >> (k + 1)), k up to first_pass_log."""
    n = 1 << log_n
    lens = {0, 1, 2, 3, n - 1, n}
    for k in range(1, first_pass_log + 2):
        lens |= {n >> k, (n >> k) - 1, (n >> k) + 1}
    return sorted(v for v in lens if 0 <= v <= n)


def skipped_stages(log_n, first_pass_log, in_len):
    """what the library's rule gives for that length (0 for an empty input: nothing is transformed)"""
    k = 0
    while in_len > 0 and k < first_pass_log and in_len <= (1 << log_n) >> (k + 1):
        k += 1
    return k


def padded(x, n):
    """x followed by zeros: what fft_with_precomputation transforms"""
    out = np.zeros((n, x.shape[1]), dtype=np.uint64)
    out[: x.shape[0]] = x
    return out
