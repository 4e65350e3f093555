"""The reference of the polynomial division and series inverse tests, on Python integers: stored words (value * 2^256 mod p) <->
canonical values, schoolbook long division, the schoolbook truncated product, the series inverse by the triangular recurrence and
Horner evaluation.  Polynomials are lists of canonical values, lowest coefficient first."""
import numpy as np

R = 1 << 256


# ---- stored words <-> Python integers ----
def words_to_ints(arr):
    b = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def ints_to_words(vals):
    if not len(vals):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(len(vals), 4).copy()


def stored(p, vals):
    return [v % p * R % p for v in vals]


def canonical(p, words):
    rinv = pow(R, -1, p)
    return [w * rinv % p for w in words]


# ---- arithmetic ----
def divide(p, a, b):
    """a: la values, b: k + 1 values with b[k] != 0, la > k -> (la - k quotient values, k remainder values): schoolbook long division"""
    k = len(b) - 1
    inv = pow(b[k], -1, p)
    rem = list(a)
    q = [0] * (len(a) - k)
    for j in range(len(a) - k - 1, -1, -1):
        c = rem[j + k] * inv % p
        q[j] = c
        if c:
            for i in range(k + 1):
                rem[j + i] = (rem[j + i] - c * b[i]) % p
    return q, rem[:k]


def mul_trunc(p, x, y, n):
    """the first n coefficients of x y"""
    out = [0] * n
    for i, u in enumerate(x[:n]):
        if u:
            for j, v in enumerate(y[:n - i]):
                out[i + j] = (out[i + j] + u * v) % p
    return out


def inverse_series(p, h, n):
    """g with g h = 1 mod X^n: g_0 = 1 / h_0, g_i = -(1 / h_0) sum_{j = 1..i} h_j g_(i - j)"""
    inv = pow(h[0], -1, p)
    g = [inv]
    for i in range(1, n):
        s = sum(h[j] * g[i - j] for j in range(1, min(i, len(h) - 1) + 1)) % p
        g.append((-inv * s) % p)
    return g


def horner(p, c, x):
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % p
    return acc


def rand_poly(p, rng, n):
    """n values: random, with planted edge values (0, 1, p - 1 and the values whose stored words are 0 / 1 / p - 1)"""
    c = [rng.randrange(p) for _ in range(n)]
    rinv = pow(R, -1, p)
    edges = [0, 1, p - 1, rinv, (p - 1) * rinv % p]
    for t in range(min(n, 10)):
        c[rng.randrange(n)] = edges[t % len(edges)]
    return c
