"""The hot-path calls of one Plonk proof (src/plonk.rs:85-200) strung together on the device, data resident in HBM
between them: 9 wire iNTTs (values_to_polynomials), 9 LDEs to 8n (polynomials_to_values_padded), 9 blinded commitments
(commit_polynomials), Z: the grand product (permutation_polynomial) + one iNTT + LDE + commitment, the vanishing polynomial (vanishing_poly: the 8n-point constraint
evaluation + one 8n iNTT), the quotient t = vanishing / Z_H (divide_by_z_h) and its 7 chunk commitments.
The witness is an honest one (ArithmeticGate / ConstantGate rows with random selector constants) with real copy constraints: the
routed wires draw their values from a small pool, every set of cells holding one value is one cycle of the wiring, and sigma maps a
cell to the next one of its cycle (hence Z is not constant, and its wrap check holds), so the numerator is a REAL vanishing polynomial and the division by Z_H is checked to be exact (q * Z_H == vanishing).
Witness generation and the transcript are not part of this probe.  With `ipa` the rounds of the opening's inner-product argument
(halo.rs:63-124) follow, over the SAME tables - built over the circuit's fixed generators [pedersen_g, pedersen_h, U] (plonk.rs:46-51)
- with stand-in challenges.  Usage (GPU box): python tools/prover_pipeline_probe.py [log_n] [ipa]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from plonky_amd import api, device as dev, synth
from plonky_amd.selfcheck import _mul
from plonky_amd.synth import MODULI

log_n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1] != "ipa" else 20
WITH_IPA = "ipa" in sys.argv
n = 1 << log_n
F, CURVE = 1, 0   # wires live in the scalar field of Tweedledee = TweedledumBase
dev.init(0)
p = MODULI[0]
G = (p - 1, 2)
D = _mul(p, 0xC0FFEE, G)
g0 = np.stack([synth.mont(0, G[0]), synth.mont(0, G[1])]); dd = np.stack([synth.mont(0, D[0]), synth.mont(0, D[1])])
gens = dev.gen_bases_dev(CURVE, n + 2, g0, dd)            # pedersen_g (n) followed by pedersen_h and U
t0 = time.perf_counter(); pre = dev.msm_precompute_dev(CURVE, gens); torch.cuda.synchronize()
print("setup: msm_precompute of %d generators %.1f ms (once per circuit)" % (n + 2, (time.perf_counter() - t0) * 1e3))

# ---- an honest witness: ArithmeticGate rows (arithmetic.rs:32-46): w3 = c0 w0 w1 + c1 w2, selector constants 1001 c0 c1 ----
ONE, ZERO = synth.mont(F, 1), synth.mont(F, 0)
w = synth.rand_field(F, 1, 9 * n).reshape(9, n, 4)
pool_rng = np.random.default_rng(3)
w[:6] = synth.rand_field(F, 4, 1024)[pool_rng.integers(0, 1024, size=6 * n)].reshape(6, n, 4)   # repeated values: copy constraints
c0, c1 = synth.rand_field(F, 7, n), synth.rand_field(F, 8, n)
w[3] = api.field_op(F, "add", api.field_op(F, "mul", api.field_op(F, "mul", c0, w[0]), w[1]), api.field_op(F, "mul", c1, w[2]))
consts = np.stack([np.tile(ONE, (n, 1)), np.tile(ZERO, (n, 1)), np.tile(ZERO, (n, 1)), np.tile(ONE, (n, 1)), c0, c1])
# odd rows: ConstantGate (constant.rs:30-39), selector constants 10110 c, w0 = c -- so that the selector polynomials are not constant
consts[2, 1::2], consts[3, 1::2], consts[4, 1::2] = ONE, ONE, ZERO
w[0, 1::2] = c1[1::2]
k_is = synth.rand_field(F, 9, 6)                                                   # get_subgroup_shift(0..5): inputs
alpha, beta, gamma = synth.rand_field(F, 10, 3)
ZETA = np.array([7605997034305223424, 3132214451552427455, 3308921103222877309, 2709928666517121162], dtype=np.uint64)  # tweedledum_curve.rs:37-44
# circuit-constant 8n tables (circuit_builder.rs:1135-1160): constants, and the wiring: the cells (j, r) of the routed wires that
# hold one value form one cycle, sigma_j[r] = k_j' g^r' of the next cell (j', r') (sigma_polynomials, plonk_util.rs:264-280)
t0 = time.perf_counter()
const_coeffs = dev.ntt_dev(F, dev.to_device(consts), inverse=True)
consts_8n = dev.ntt_padded_dev(F, const_coeffs, log_n + 3)
sig = np.zeros((6, n, 4), dtype=np.uint64); sig[:, 1] = k_is
ident = dev.to_host(dev.ntt_dev(F, dev.to_device(sig))).reshape(6 * n, 4)          # k_j g^r, row r
key = np.unique(np.ascontiguousarray(w[:6]).reshape(6 * n, 4).view("V32").ravel(), return_inverse=True)[1].ravel()
order = np.argsort(key, kind="stable")
ks = key[order]
new_group = np.insert(ks[1:] != ks[:-1], 0, True)
first = np.maximum.accumulate(np.where(new_group, np.arange(6 * n), 0))
succ = np.arange(1, 6 * n + 1)
last = np.append(new_group[1:], True)
succ[last] = first[last]
nxt = np.empty(6 * n, dtype=np.int64); nxt[order] = order[succ]
sigma_n = dev.to_device(ident[nxt].reshape(6, n, 4))
sigma_8n = dev.ntt_padded_dev(F, dev.ntt_dev(F, sigma_n, inverse=True), log_n + 3)   # s_sigma_values_8n
torch.cuda.synchronize()
print("setup: constants_8n / s_sigma_values_8n %.1f ms (once per circuit)" % ((time.perf_counter() - t0) * 1e3))
wires = dev.to_device(w)
blind = torch.cat([dev.to_device(synth.rand_field(F, 2, 9 + 1 + 7)).reshape(-1, 1, 4), torch.zeros((17, 1, 4), dtype=torch.int64, device="cuda")], dim=1)  # [r] H + [0] U
zvals = torch.empty((n, 4), dtype=torch.int64, device="cuda")
zstatus = torch.empty(2, dtype=torch.int32, device="cuda")
t_out = torch.empty((8 * n, 4), dtype=torch.int64, device="cuda")
ev8 = torch.empty((9, 8 * n, 4), dtype=torch.int64, device="cuda")
pts = torch.empty((8 * n, 4), dtype=torch.int64, device="cuda")
t7 = torch.zeros((7 * n, 4), dtype=torch.int64, device="cuda")


def run():
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(9)]
    marks[0].record()
    polys = dev.ntt_dev(F, wires, inverse=True)                                     # values_to_polynomials
    marks[1].record()
    dev.ntt_padded_dev(F, polys, log_n + 3, out=ev8)                                # polynomials_to_values_padded
    marks[2].record()
    c_wires = dev.msm_execute_dev(pre, torch.cat([polys, blind[:9]], dim=1).contiguous())   # commit_polynomials (+ [r] H)
    marks[3].record()
    dev.permutation_polynomial_dev(F, log_n, wires, sigma_8n, k_is, beta, gamma, sigma_stride=8, out=zvals, status=zstatus)   # plonk.rs:127-134
    marks[8].record()
    zpoly = dev.ntt_dev(F, zvals, inverse=True)
    z_8n = dev.ntt_padded_dev(F, zpoly, log_n + 3)                                  # plonk.rs:388-391
    c_z = dev.msm_execute_dev(pre, torch.cat([zpoly, blind[9]], dim=0).contiguous())
    marks[4].record()
    dev.vanishing_points_dev(F, log_n, consts_8n, ev8, sigma_8n, z_8n, k_is, alpha, beta, gamma, ZETA, ZERO, out=pts)   # plonk.rs:392-453
    marks[5].record()
    vanishing = dev.ntt_dev(F, pts, inverse=True)                                   # Polynomial::from_evaluations, plonk.rs:455
    t = dev.divide_by_z_h_dev(F, vanishing, n, out=t_out)                           # quotient, plonk.rs:178-181
    marks[6].record()
    t7.zero_()
    t7[: min(t.shape[0], 7 * n)] = t[: 7 * n]                                      # plonk.rs:182: pad to 7n, split
    chunks = t7.reshape(7, n, 4)
    c_t = dev.msm_execute_dev(pre, torch.cat([chunks, blind[10:17]], dim=1).contiguous())
    marks[7].record()
    torch.cuda.synchronize()
    names = ["9 wire iNTT (n)", "9 LDE n -> 8n", "9 wire commitments", "Z: grand product (n, stride 8)", "Z: iNTT + LDE + commitment",
             "vanishing points (8n, 10 gates)", "iNTT (8n) + divide_by_z_h", "7 quotient-chunk commitments"]
    seq = [0, 1, 2, 3, 8, 4, 5, 6, 7]
    ms = [marks[seq[i]].elapsed_time(marks[seq[i + 1]]) for i in range(8)]
    return names, ms, t, vanishing


run()
names, ms, t, vanishing = run()
q = dev.to_host(t7)
v = dev.to_host(vanishing)
zpad = np.zeros((n, 4), dtype=np.uint64)
back = api.field_op(F, "sub", np.concatenate([zpad, q]), np.concatenate([q, zpad]))   # q * (X^n - 1)
ok = bool(v.any() and not dev.to_host(t)[7 * n:].any() and np.array_equal(back, v))
zh = dev.to_host(zvals)
print("Z: status %s (zero denominators, wraps to 1), distinct values among the first 1024 rows: %d" % (zstatus.cpu().tolist(), len({r.tobytes() for r in zh[:1024]})))
print("q * Z_H == vanishing: %s" % ok)
for nm, tv in zip(names, ms):
    print("  %-34s %8.3f ms" % (nm, tv))
print("hot-path device time per proof at n = 2^%d: %.2f ms   (real numerator; q * Z_H == vanishing polynomial, deg q < 7n: %s)" % (log_n, sum(ms), ok))
if WITH_IPA:
    r = MODULI[F]
    m1 = lambda v: np.array(synth.mont(F, v), dtype=np.uint64)
    x_int = 0x1F3D5B79A2C4E6081F3D5B79A2C4E6081F3D5B79A2C4E608 % r          # halo_n(u_scaling bits): u_prime = [x] U
    k_u, k_h = (1 + (n + 1) * 0xC0FFEE) % r, (1 + n * 0xC0FFEE) % r            # generator i is G0 + i D = [1 + i 0xC0FFEE] G0
    pm = lambda P: np.stack([synth.mont(0, P[0]), synth.mont(0, P[1])])
    Hm, Upm = pm(_mul(p, k_h, G)), pm(_mul(p, x_int * k_u % r, G))
    us = [synth.to_int(row) % r or 1 for row in synth.rand_field(F, 31, log_n)]
    ums = [(m1(u), m1(pow(u, -1, r))) for u in us]
    bl = [(m1(100 + j), m1(200 + j)) for j in range(log_n)]
    # the opening (plonk.rs:261-308, halo.rs:38-47): the 30 polynomials - 6 constants, 6 sigmas, 9 wires, Z, 7 chunks of t, and the
    # public-input quotient (plonk.rs:199-235, k = 2 public-input rows) - at zeta, zeta g, zeta g^65; then halo_a, halo_b
    polys = dev.ntt_dev(F, wires, inverse=True)
    sigma_coeffs = dev.ntt_dev(F, sigma_n, inverse=True)
    zpoly = dev.ntt_dev(F, zvals, inverse=True)
    opened = [const_coeffs[i] for i in range(6)] + [sigma_coeffs[i] for i in range(6)] + [polys[i] for i in range(9)] + [zpoly] + \
             [t7[i * n:(i + 1) * n] for i in range(7)]
    gsub = np.zeros((n, 4), dtype=np.uint64); gsub[1] = ONE
    g_n = synth.from_mont(F, dev.to_host(dev.ntt_dev(F, dev.to_device(gsub))[1]))          # the generator of the n-subgroup
    # the wire values without public inputs are zero at the public-input rows (plonk.rs:109-118): rows 0 and 1 here, the subgroup
    # points 1 and g; their polynomials, scaled by powers of alpha, divided by (X - 1)(X - g) (plonk.rs:199-235)
    PI_ROWS = 2
    wires_no_pis = wires.clone()
    wires_no_pis[:, :PI_ROWS] = 0
    polys_no_pis = dev.ntt_dev(F, wires_no_pis, inverse=True)
    pi_roots = np.stack([m1(pow(g_n, i, r)) for i in range(PI_ROWS)])
    pe = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(2):
        pe[0].record()
        pi_quotient, pi_rem = dev.public_input_quotient_dev(F, [polys_no_pis[i] for i in range(9)], alpha, pi_roots, n)
        pe[1].record()
    torch.cuda.synchronize()
    pi_ok = bool(not dev.to_host(pi_rem).any() and dev.to_host(pi_quotient).any())
    print("  %-34s %8.3f ms   remainder is zero: %s" % ("public-input quotient (k = %d)" % PI_ROWS, pe[0].elapsed_time(pe[1]), pi_ok))
    assert pi_ok, "the public-input quotient left a remainder"
    opened.append(pi_quotient)
    assert len(opened) == 30
    zeta_int = synth.to_int(synth.rand_field(F, 34, 1)[0]) % r
    open_pts = np.stack([m1(zeta_int), m1(zeta_int * g_n % r), m1(zeta_int * pow(g_n, 65, r) % r)])
    s_ints = [synth.to_int(row) % r for row in synth.rand_field(F, 35, 30)]                 # u^i: stand-in challenges
    v_int = synth.to_int(synth.rand_field(F, 36, 1)[0]) % r
    s_m = np.stack([m1(x) for x in s_ints])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for _ in range(2):
        ev[0].record()
        o = dev.eval_polys_dev(F, opened, open_pts)
        ev[1].record()
        halo_a = dev.reduce_polynomials_dev(F, opened, s_m, n)
        ev[2].record()
        halo_b = dev.build_halo_b_dev(F, open_pts, m1(v_int), n)
        ev[3].record()
    torch.cuda.synchronize()
    open_ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(3)]
    for nm, tv in zip(("opening: 30 polys at 3 points", "opening: reduced polynomial halo_a", "opening: halo_b"), open_ms):
        print("  %-34s %8.3f ms" % (nm, tv))
    # <halo_a, halo_b> = sum_k v^k sum_i s_i o[k][i]: the identity that ties the three results together, checked on the device's outputs
    o_int = [[synth.from_mont(F, row) for row in pt] for pt in dev.to_host(o)]
    rhs = sum(pow(v_int, k, r) * sum(s * x for s, x in zip(s_ints, o_int[k])) for k in range(3)) % r
    lhs = synth.from_mont(F, dev.to_host(dev.inner_product_dev(F, halo_a, halo_b))[0])
    assert lhs == rhs, "<halo_a, halo_b> != sum_k v^k sum_i s_i o[k][i]"
    print("  <halo_a, halo_b> == sum_k v^k sum_i s_i o[k][i]: True")
    g_only = gens[:n].contiguous()
    def ipa():
        t0 = time.perf_counter()
        arg = dev.HaloArgument(CURVE, halo_a, halo_b, g_only, Hm, Upm, tables=pre, h_index=n, u_index=n + 1, u_prime_scalar=m1(x_int))
        for j in range(log_n):
            t1 = time.perf_counter()
            arg.round_lr(*bl[j])
            t2 = time.perf_counter()
            arg.round_fold(*ums[j])
            if os.environ.get("PROBE_ROUNDS"):
                torch.cuda.synchronize()
                print("    round at length %8d: L/R %.3f ms  fold %.3f ms" % (len(arg) * 2, (t2 - t1) * 1e3, (time.perf_counter() - t2) * 1e3))
        fin = arg.read()
        t = time.perf_counter() - t0
        arg.free()
        return t, fin
    ipa()
    t_ipa, _ = ipa()
    print("  %-34s %8.3f ms   (%d rounds over the same tables; wall clock of the loop, every round ends on the host)" % ("inner-product argument", t_ipa * 1e3, log_n))
    print("hot path of one proof incl. the opening: %.2f ms" % (sum(ms) + sum(open_ms) + t_ipa * 1e3))
