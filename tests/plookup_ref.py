"""Big-integer restatements of the two loops of the Plookup prover (plookup/src/plookup.rs) that run on the device:
grand_polynomial (plookup.rs:180-202) and the 4(n+1)-point loop of vanishing_polynomial (plookup.rs:225-269), with eval_l_i
(plookup.rs:275-282) as the reference writes it - including its ZERO at x == g.  Plain Python integers, canonical values;
the field constants come from oracle.bigint_ref."""
from oracle import bigint_ref as br  # noqa: F401  (FieldSpec: p, primitive_root_of_unity)


def sort_by(f, t):
    """plookup.rs:171-177: a stable sort of f on the position of each element's first occurrence in t"""
    return sorted(f, key=lambda a: t.index(a))


def grand_polynomial(fs, f, t, s, beta, gamma):
    """plookup.rs:180-202 on canonical ints, row by row: f has n values, t n + 1, s 2 n + 1.  Returns (values, status) with the status
    words of the device entry: zero denominators among rows 0..n-2 (where the reference's `/` panics; the row's denominator is
    then taken as 1, as the device does), and whether no row 0..n-1 had one and the product over all n rows is 1."""
    p, n = fs.p, len(f)
    assert len(t) == n + 1 and len(s) == 2 * n + 1
    beta1 = (beta + 1) % p
    gamma_beta1 = gamma * beta1 % p
    values, total, zeros, clean = [1], 1, 0, True
    for j in range(n):
        num = beta1 * (gamma + f[j]) % p * (gamma_beta1 + t[j] + beta * t[j + 1]) % p
        den = (gamma_beta1 + s[j] + beta * s[j + 1]) * (gamma_beta1 + s[n + j] + beta * s[n + j + 1]) % p
        if den == 0:
            zeros += j < n - 1
            clean = False
            den = 1
        total = total * num * pow(den, -1, p) % p
        if j < n - 1:
            values.append(total)
    values.append(1)  # plookup.rs:200
    return values, [zeros, int(clean and total == 1)]


def eval_l_i(fs, n, i, generator, x):
    """plookup.rs:275-282"""
    p = fs.p
    g = pow(generator, i, p)
    if x == g:
        return 0
    return g * (pow(x, n, p) - 1) * pow(n * (x - g), -1, p) % p


def vanishing_values(fs, log_size, z, f, t, h1, h2, alpha, beta, gamma):
    """plookup.rs:225-269: the five rows are the values on the 4(n+1) domain; returns the 4(n+1) values"""
    p = fs.p
    size = 1 << log_size
    n, order = size - 1, 4 * size
    g4 = fs.primitive_root_of_unity(log_size + 2)
    w = pow(g4, 4, p)
    last_root = pow(g4, 4 * n, p)
    beta1 = (beta + 1) % p
    gamma_beta1 = gamma * beta1 % p
    out, x = [], 1
    for i in range(order):
        nxt = (i + 4) % order
        z1 = eval_l_i(fs, size, 0, w, x) * (z[i] - 1) % p
        shift = ((x - last_root) * z[i] * beta1 * (gamma + f[i]) * (gamma_beta1 + t[i] + beta * t[nxt])
                 - (x - last_root) * z[nxt] * (gamma_beta1 + h1[i] + beta * h1[nxt]) * (gamma_beta1 + h2[i] + beta * h2[nxt])) % p
        eval_last = eval_l_i(fs, size, n, w, x)
        hs = eval_last * (h1[i] - h2[nxt]) % p
        last = eval_last * (z[i] - 1) % p
        acc = 0
        for term in (last, hs, shift, z1):  # reduce_with_powers, plonk_util.rs:27-33
            acc = (acc * alpha + term) % p
        out.append(acc)
        x = x * g4 % p
    return out
