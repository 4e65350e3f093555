// plookup.hip -- the two O(n) loops of the Plookup prover on the device (plookup/src/plookup.rs::prove; everything else of `prove` maps
// onto the transforms, commitments, division and opening entry points - INTEGRATION.md has the call-by-call map).
//
// Reference path                                                              here
//   grand_polynomial, the serial prefix product        plookup.rs:180-202  ->  k_lookup_rows, k_perm_tiles (lz.cuh), k_lookup_fix
//   vanishing_polynomial, the 4(n+1)-point loop        plookup.rs:225-269  ->  k_lookup_points
//   eval_l_i                                           plookup.rs:275-282  ->  a cached table of L_0 over the 4(n+1) domain
//   reduce_with_powers                                 plonk_util.rs:27-33 ->  inside k_lookup_points
// N = n + 1 = 2^log_size is the order of the subgroup H, w its generator, g4 the primitive 4N-th root (g4^4 = w).
//
// eval_l_i returns ZERO when x equals the basis point itself (it tests x == g before it divides), and x^N - 1 vanishes at every other
// point of H, so BOTH Lagrange factors are 0 at every i = 0 (mod 4) of the 4N domain.  Elsewhere L_0(x) = (x^N - 1) / (N (x - 1)), and
// because w^N = 1, L_n(x) = w^n (x^N - 1) / (N (x - w^n)) = L_0(x w): the factor eval_l_i(N, n, w, g4^i) is the L_0 table at index
// (i + 4) mod 4N - the same `next` the shifted rows are read at.  One table serves both factors.
//
// The arithmetic is the Lz working form of lz.cuh: exact modulo p, reduced to the unique representative at the end, so the results
// are bit-identical to the reference's whatever the grouping.
#include <memory>
#include <tuple>
#include <utility>

#include "common.h"
#include "fp.cuh"
#include "tables.cuh"
#include "lz.cuh"

namespace plk {

// per-row / per-point arrays are indexed at compile time (a run-time index puts the array in scratch memory)
template <class F, int... I> PLK_DI void lkp_static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F> PLK_DI void lkp_static_for(F&& f) { lkp_static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// ---------------------------------------------------------------------------------------------
// tables (device, field, log of the domain): powers of g4 in both forms, L_0 over the domain, the table of lz_from_rform
// ---------------------------------------------------------------------------------------------
struct LookupTables : DomainTables {  // the domain of g4; `small` is not read here
    DevBuf l0;                        // eval_l_i(N, 0, w, g4^i), i < 4N, R'-form; 0 at every i = 0 (mod 4)
};
static TableCache<std::tuple<int, int, int>, LookupTables> g_lookup;

// N (x - 1) for the batch inversion, R-form; 1 where the table is 0 anyway (x = 1 has no inverse)
template <class P> __global__ void __launch_bounds__(128) k_lookup_l0_den(const uint4* __restrict__ lo, const uint4* __restrict__ hi, int log_size,
                                                                          uint4* __restrict__ den) {
    const size_t n4 = (size_t)4 << log_size;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const Fe<P> one = fe_one<P>();
    Fe<P> nf = fe_zero<P>();
    nf.v[log_size >> 5] = 1u << (log_size & 31);
    nf = fe_from_canonical<P>(nf);  // from_canonical_usize(N)
    fe_store<P>(den + i * 2, (i & 3) == 0 ? one : fe_mul<P>(nf, fe_sub<P>(plonk_x<P>(lo, hi, i), one)));
}
// in place: 1 / (N (x - 1)) -> L_0(x) in R'-form.  x^N = g4^(N i) = g4^(N (i mod 4)): four values over the domain
template <class P> __global__ void __launch_bounds__(128) k_lookup_l0(const uint4* __restrict__ lo, const uint4* __restrict__ hi, int log_size, uint4* l0) {
    const size_t n4 = (size_t)4 << log_size;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    Fe<P> r = fe_zero<P>();
    if ((i & 3) != 0) r = fe_mul<P>(fe_sub<P>(plonk_x<P>(lo, hi, (i & 3) << log_size), fe_one<P>()), fe_load<P>(l0 + i * 2));
    fe_store<P>(l0 + i * 2, to_rprime<P>(r));
}

// log_size = 0: the size-independent part only (the grand product reads nothing else)
template <class P> static int get_lookup_tables(int log_size, hipStream_t stream, std::shared_ptr<LookupTables>& out) {
    int dev = 0;
    PLK_HIP_TRY(hipGetDevice(&dev));
    return g_lookup.get(std::make_tuple(dev, (int)P::FIELD_ID, log_size), out, [&](LookupTables& t) {
        const bool points = log_size > 0;
        const int log_n4 = points ? log_size + 2 : XS_LO_LOG;
        const size_t n4 = (size_t)1 << log_n4;
        std::shared_ptr<const void> plan_hold;  // keeps the plan (and its power table) alive across the launches
        PLK_TRY(build_domain_tables<P>(log_n4, stream, t, plan_hold));
        if (points) {
            PLK_TRY(t.l0.alloc(n4 * 32));
            ScratchSet ss(stream);
            void* den = ss.get(n4 * 32);
            if (!den) return PLK_ERR_OOM;
            const unsigned blocks = (unsigned)((n4 + 127) / 128);
            k_lookup_l0_den<P><<<blocks, 128, 0, stream>>>((const uint4*)t.xs_lo.p, (const uint4*)t.xs_hi.p, log_size, (uint4*)den);
            PLK_HIP_TRY(hipGetLastError());
            PLK_TRY(field_batch_inverse_dev_impl(P::FIELD_ID, den, t.l0.p, nullptr, nullptr, n4, stream));
            k_lookup_l0<P><<<blocks, 128, 0, stream>>>((const uint4*)t.xs_lo.p, (const uint4*)t.xs_hi.p, log_size, (uint4*)t.l0.p);
            PLK_HIP_TRY(hipGetLastError());
        }
        PLK_HIP_TRY(hipStreamSynchronize(stream));  // the power table of the plan is only borrowed for these launches
        return PLK_OK;
    });
}

// ---------------------------------------------------------------------------------------------
// the scalars of a call, in the working form: one lane, once per call; the kernels stage the rows in LDS
// ---------------------------------------------------------------------------------------------
struct LookupScalars {
    uint32_t alpha[8], beta[8], gamma[8];
};
// row: value (bound in eighths of p)
constexpr int LKP_ALPHA = 0, LKP_BETA = 1, LKP_GAMMA = 2;  // as given (16)
constexpr int LKP_BETA1 = 3;                               // beta + 1 (24)
constexpr int LKP_GAMMA_BETA1 = 4;                         // gamma (beta + 1) (9)
constexpr int LKP_ALPHA2 = 5, LKP_ALPHA3 = 6;              // (9)
constexpr int LKP_X_LAST = 7;                              // g4^(4 n) = w^n, the root the shift term divides out (9); points only
constexpr int LKP_SCALARS = 8;
template <class P> __global__ void __launch_bounds__(64) k_lookup_scalars(LookupScalars sc, const uint4* __restrict__ xs_lo_z, const uint4* __restrict__ xs_hi_z,
                                                                          size_t i_last, uint32_t* __restrict__ out) {
    constexpr int NZ = FzCfg<P>::NZ;
    if (threadIdx.x != 0) return;
    auto load = [](const uint32_t (&w)[8]) {
        Fe<P> x;
#pragma unroll
        for (int i = 0; i < 8; ++i) x.v[i] = w[i];
        return lz_from_rform<P>(x);
    };
    auto put = [&](int row, const Fz<P>& v) {
#pragma unroll
        for (int i = 0; i < NZ; ++i) out[row * NZ + i] = v.l[i];
    };
    const auto alpha = load(sc.alpha), beta = load(sc.beta), gamma = load(sc.gamma);
    const auto beta1 = beta + lz_one<P>();
    const auto alpha2 = alpha * alpha;
    put(LKP_ALPHA, alpha.v);
    put(LKP_BETA, beta.v);
    put(LKP_GAMMA, gamma.v);
    put(LKP_BETA1, beta1.v);
    put(LKP_GAMMA_BETA1, (gamma * beta1).v);
    put(LKP_ALPHA2, alpha2.v);
    put(LKP_ALPHA3, (alpha2 * alpha).v);
    if (xs_lo_z) put(LKP_X_LAST, (lz_table<P>(xs_lo_z, i_last & (((size_t)1 << XS_LO_LOG) - 1)) * lz_table<P>(xs_hi_z, i_last >> XS_LO_LOG)).v);
    else put(LKP_X_LAST, fz_zero<P>());
}
// global -> LDS; ends with the barrier that publishes the rows (and whatever the caller staged before)
template <class P> PLK_DI void lkp_stage_scalars(const uint32_t* __restrict__ scal, uint32_t (*s_sc)[FzCfg<P>::NZ]) {
    constexpr int NZ = FzCfg<P>::NZ;
    for (int k = threadIdx.x; k < LKP_SCALARS * NZ; k += blockDim.x) s_sc[k / NZ][k % NZ] = scal[k];
    __syncthreads();
}
template <int B, class P> PLK_DI Lz<P, B> lkp_scalar(const uint32_t (*s_sc)[FzCfg<P>::NZ], int row) {
    Lz<P, B> r;
#pragma unroll
    for (int i = 0; i < FzCfg<P>::NZ; ++i) r.v.l[i] = s_sc[row][i];
    return r;
}

// ---------------------------------------------------------------------------------------------
// grand_polynomial (plookup.rs:180-202)
// ---------------------------------------------------------------------------------------------
// values[i] = prod_(j < i) r_j with r_j = beta1 (gamma + f_j) (gb1 + t_j + beta t_(j+1)) / [(gb1 + s_j + beta s_(j+1)) (gb1 + s_(n+j) + beta s_(n+j+1))]
// (beta1 = beta + 1, gb1 = gamma beta1): the EXCLUSIVE product scan of r over rows 0..n-1, with values[n] forced to ONE as the reference
// pushes it.  Reduce-then-scan in the shape of the permutation Z (plonk.hip):
//   k_lookup_rows  a lane owns LKP_ROWS consecutive rows: num / den of each, ONE inversion for the lane (Montgomery's trick on the prefix
//                  products), then a workgroup scan of the lane totals; writes the tile-local exclusive prefixes (R'-form words) and a tile total;
//   k_perm_tiles   (lz.cuh) scans the tile totals and writes the status words;
//   k_lookup_fix   values[i] = tile prefix x local prefix in the reference's form; values[n] = 1.
// A lane reads t_j, s_j, s_(n+j) once: the row after takes them over.  Row N - 1 does not exist (num = den = 1).  A zero den is replaced
// by 1 and counted: rows 0..n-2 are the reference's panic, row n - 1 only spoils the closing check.
constexpr int LKP_ROWS = 4, LKP_LANES = 128, LKP_TILE = LKP_ROWS * LKP_LANES;

template <class P>
__global__ void __launch_bounds__(LKP_LANES) k_lookup_rows(const uint4* __restrict__ f, const uint4* __restrict__ t, const uint4* __restrict__ s,
                                                          const uint32_t* __restrict__ scal, size_t n, uint4* __restrict__ out,
                                                          uint32_t* __restrict__ tile_tot, unsigned* __restrict__ zeros, const uint32_t* __restrict__ top_table) {
    static_assert(P::NL == 8, "256-bit scalar fields");
    constexpr int NZ = FzCfg<P>::NZ;
    using D = Lz<P, 16>;
    __shared__ uint32_t s_sc[LKP_SCALARS][NZ];
    __shared__ uint32_t s_wave[LKP_LANES / 64][NZ];
    __shared__ __attribute__((aligned(16))) LzTop<P> s_top;
    stage_top_table<P>(top_table, s_top);
    lkp_stage_scalars<P>(scal, s_sc);
    const size_t r0 = ((size_t)blockIdx.x * LKP_LANES + threadIdx.x) * LKP_ROWS;
    const auto beta = lkp_scalar<16, P>(s_sc, LKP_BETA), gamma = lkp_scalar<16, P>(s_sc, LKP_GAMMA);
    const auto beta1 = lkp_scalar<24, P>(s_sc, LKP_BETA1);
    const LzP<P> gb1 = lkp_scalar<9, P>(s_sc, LKP_GAMMA_BETA1);
    const LzP<P> one = lz_one<P>().template widen<9>();
    using Den = Lz<P, lz_mul_bound(34, 34)>;  // a product of two factors below (34 / 8) p
    LzP<P> num_pre[LKP_ROWS];  // num_pre[m] = N_(m+1) = prod_(k <= m) num_k
    Den den[LKP_ROWS];
    LzP<P> n_run = one, d_run = one;
    D t_cur{fz_zero<P>()}, s_cur{fz_zero<P>()}, h_cur{fz_zero<P>()};  // t_j, s_j, s_(n+j) of the row at hand
    if (r0 < n) {
        t_cur = lz_load<P>(t, r0, s_top);
        s_cur = lz_load<P>(s, r0, s_top);
        h_cur = lz_load<P>(s, n + r0, s_top);
    }
    unsigned z_head = 0, z_last = 0;
    lkp_static_for<LKP_ROWS>([&](auto M) {
        constexpr int m = decltype(M)::value;
        const size_t r = r0 + m;
        LzP<P> num = one;
        Den de = one.template widen<lz_mul_bound(34, 34)>();
        if (r < n) {
            const D t_nx = lz_load<P>(t, r + 1, s_top), s_nx = lz_load<P>(s, r + 1, s_top), h_nx = lz_load<P>(s, n + r + 1, s_top);
            const D fj = lz_load<P>(f, r, s_top);
            num = (beta1 * (gamma + fj)) * (gb1 + t_cur + beta * t_nx);
            de = (gb1 + s_cur + beta * s_nx) * (gb1 + h_cur + beta * h_nx);
            t_cur = t_nx;
            s_cur = s_nx;
            h_cur = h_nx;
            if (fz_is_zero_mod_p<P>(de.v)) {  // field.rs "No inverse" for rows 0..n-2
                de = one.template widen<lz_mul_bound(34, 34)>();
                if (r + 1 < n) ++z_head;
                else ++z_last;
            }
        }
        n_run = n_run * num;
        num_pre[m] = n_run;
        den[m] = de;
        d_run = d_run * de;
    });
    // 1 / D_ROWS through the reference's form (the inversion works on the integer), back to R'-form limbs
    // (inlined here: as a call the inversion takes its operand through private memory, the kernel's only scratch)
    const Fe<P> d_total = lz_to_rform<P>(d_run);
    Fe<P> d_inv;
    [[clang::always_inline]] d_inv = fe_inv_safegcd_impl<P, 0>(d_total);
    LzP<P> inv = Lz<P, 8>{fz_from_fe<P>(d_inv)} * Lz<P, 8>{fz_const_r_to_rprime<P>()};
    const LzP<P> lane_total = num_pre[LKP_ROWS - 1] * inv;
    LzP<P> e[LKP_ROWS];  // e[m] = N_m / D_m: the product of r over the lane's rows before m
    e[0] = one;
    lkp_static_for<LKP_ROWS - 1>([&](auto I) {
        constexpr int m = LKP_ROWS - 1 - decltype(I)::value;
        inv = inv * den[m];  // 1 / D_m
        e[m] = num_pre[m - 1] * inv;
    });
    if (z_head) atomicAdd(&zeros[0], z_head);
    if (z_last) atomicAdd(&zeros[1], z_last);
    const LzP<P> ex = wg_exclusive_product<P, LKP_LANES / 64>(lane_total, s_wave);
    if (threadIdx.x == LKP_LANES - 1) limbs_store<P>(tile_tot, blockIdx.x, (ex * lane_total).v);
    lkp_static_for<LKP_ROWS>([&](auto M) {
        constexpr int m = decltype(M)::value;
        if (r0 + m <= n) {  // row n holds the total until k_lookup_fix puts ONE there
            const LzP<P> v = m == 0 ? ex : ex * e[m];
            fe_store<P>(out + (r0 + m) * 2, fz_to_fe_canonical<P>(v.v));  // R'-form words, canonical (k_lookup_fix reads them back)
        }
    });
}

template <class P> __global__ void __launch_bounds__(256) k_lookup_fix(uint4* __restrict__ out, const uint32_t* __restrict__ tile_pre, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {  // plookup.rs:200
        fe_store<P>(out + i * 2, fe_one<P>());
        return;
    }
    const LzP<P> z = lz_table<P>(out, i) * LzP<P>{limbs_load<P>(tile_pre, i / LKP_TILE)};
    fe_store<P>(out + i * 2, fz_to_fe_canonical<P>(z.v));
}

static void fill_lookup_scalars(LookupScalars& sc, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma) {
    static const uint64_t zero4[4] = {0, 0, 0, 0};
    limbs_to_words(sc.alpha, alpha ? alpha : zero4);
    limbs_to_words(sc.beta, beta);
    limbs_to_words(sc.gamma, gamma);
}

template <class P>
static int grand_product_t(unsigned log_size, const void* d_f, const void* d_t, const void* d_s, const LookupScalars& sc, void* d_out, void* d_status,
                           hipStream_t stream) {
    std::shared_ptr<LookupTables> tb;
    PLK_TRY(get_lookup_tables<P>(0, stream, tb));
    const size_t N = (size_t)1 << log_size, n = N - 1, tiles = (N + LKP_TILE - 1) / LKP_TILE;
    ScratchSet ss(stream);
    unsigned* zeros = (unsigned*)ss.get(2 * sizeof(unsigned));
    uint32_t* tile_tot = (uint32_t*)ss.get(limb_bytes(tiles, FzCfg<P>::NZ));
    uint32_t* scal = (uint32_t*)ss.get((size_t)LKP_SCALARS * FzCfg<P>::NZ * 4);
    if (!zeros || !tile_tot || !scal) return PLK_ERR_OOM;
    hipError_t e = hipMemsetAsync(zeros, 0, 2 * sizeof(unsigned), stream);
    if (e == hipSuccess) {
        k_lookup_scalars<P><<<1, 64, 0, stream>>>(sc, nullptr, nullptr, 0, scal);
        k_lookup_rows<P><<<(unsigned)tiles, LKP_LANES, 0, stream>>>((const uint4*)d_f, (const uint4*)d_t, (const uint4*)d_s, scal, n, (uint4*)d_out, tile_tot, zeros,
                                                                    (const uint32_t*)tb->top.p);
        k_perm_tiles<P><<<1, PERM_SCAN_LANES, 0, stream>>>(tile_tot, tiles, zeros, (uint32_t*)d_status);
        k_lookup_fix<P><<<(unsigned)((N + 255) / 256), 256, 0, stream>>>((uint4*)d_out, tile_tot, n);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "plookup grand product launch failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

int plookup_grand_product_dev_impl(unsigned log_size, int field, const void* d_f, const void* d_t, const void* d_s, const uint64_t* beta, const uint64_t* gamma,
                                   void* d_out, void* d_status, hipStream_t stream) {
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a circuit scalar field", field);
    if (log_size == 0) return set_error(PLK_ERR_INVALID_ARG, "log_size 0: the grand product reads f[0] (plookup.rs:187)");
    if (log_size > 28) return set_error(PLK_ERR_TWO_ADICITY, "log_size %u too large", log_size);
    if (!d_f || !d_t || !d_s || !d_out) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    if (!beta || !gamma) return set_error(PLK_ERR_INVALID_ARG, "null challenge pointer");
    PLK_TRY(ensure_device());
    LookupScalars sc;
    fill_lookup_scalars(sc, nullptr, beta, gamma);
    return or_invalid(with_field4(field, [&](auto t) { return grand_product_t<tag_t<decltype(t)>>(log_size, d_f, d_t, d_s, sc, d_out, d_status, stream); }),
                      "field %d is not a circuit scalar field", field);
}

// ---------------------------------------------------------------------------------------------
// vanishing_polynomial's loop (plookup.rs:225-269): one lane per point of the 4N domain
// ---------------------------------------------------------------------------------------------
// With x = g4^i, next = (i + 4) mod 4N, l0 = L_0(x), ln = L_n(x) = the L_0 table at `next`, xm = x - w^n:
//   z1 = l0 (z - 1)
//   shift = xm [z beta1 (gamma + f) (gb1 + t + beta t') - z' (gb1 + h1 + beta h1') (gb1 + h2 + beta h2')]      (' = at next)
//   hs = ln (h1 - h2'),  last = ln (z - 1)
//   out = z1 + alpha shift + alpha^2 hs + alpha^3 last  =  l0 (z - 1) + alpha shift + ln [alpha^2 (h1 - h2') + alpha^3 (z - 1)]
// Sums of products go through one reduction each (LzWide): 11 products and 3 reductions a point, one product for x.
// A point reads 9 rows x 32 B, two L_0 entries and writes 32 B: 384 B by count (the two x factors come from tables that stay in cache).
template <class P>
__global__ void __launch_bounds__(128) k_lookup_points(const uint4* __restrict__ values, const uint4* __restrict__ xs_lo_z, const uint4* __restrict__ xs_hi_z,
                                                       const uint4* __restrict__ l0_tab, const uint32_t* __restrict__ scal, int log_size, uint4* __restrict__ out,
                                                       const uint32_t* __restrict__ top_table) {
    static_assert(P::NL == 8, "256-bit scalar fields");
    constexpr int NZ = FzCfg<P>::NZ;
    using D = Lz<P, 16>;
    __shared__ uint32_t s_sc[LKP_SCALARS][NZ];
    __shared__ __attribute__((aligned(16))) LzTop<P> s_top;
    stage_top_table<P>(top_table, s_top);
    lkp_stage_scalars<P>(scal, s_sc);
    const size_t n4 = (size_t)4 << log_size;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const size_t next = (i + 4) & (n4 - 1);
    const auto beta = lkp_scalar<16, P>(s_sc, LKP_BETA), gamma = lkp_scalar<16, P>(s_sc, LKP_GAMMA);
    const auto beta1 = lkp_scalar<24, P>(s_sc, LKP_BETA1);
    const auto gb1 = lkp_scalar<9, P>(s_sc, LKP_GAMMA_BETA1);
    const auto one = lz_one<P>();
    const auto zero = Lz<P, 0>{fz_zero<P>()};
    // rows z, f, t, h1, h2 of the LDE table (plookup.rs:219-223)
    const D z_x = lz_load<P>(values, i, s_top), z_nx = lz_load<P>(values, next, s_top);
    const auto num = (beta1 * (gamma + lz_load<P>(values, n4 + i, s_top))) * (gb1 + lz_load<P>(values, 2 * n4 + i, s_top) + beta * lz_load<P>(values, 2 * n4 + next, s_top));
    const D h1_x = lz_load<P>(values, 3 * n4 + i, s_top);
    const D h2_nx = lz_load<P>(values, 4 * n4 + next, s_top);
    const auto den = (gb1 + h1_x + beta * lz_load<P>(values, 3 * n4 + next, s_top)) * (gb1 + lz_load<P>(values, 4 * n4 + i, s_top) + beta * h2_nx);
    // z num - z' den: two products, one reduction (z / z' are rows as loaded: two column units each)
    const auto inner = lz_reduce(lz_mac<false, true>(lz_mac<false, true>(lz_wide<P>(), num, z_x), zero - den, z_nx));
    const auto x = lz_table<P>(xs_lo_z, i & (((size_t)1 << XS_LO_LOG) - 1)) * lz_table<P>(xs_hi_z, i >> XS_LO_LOG);  // hi[0] = 1
    const auto shift = (x - lkp_scalar<9, P>(s_sc, LKP_X_LAST)) * inner;
    const auto z_m1 = z_x - one;
    const auto tail = lz_reduce(lz_mac(lz_mac(lz_wide<P>(), lkp_scalar<9, P>(s_sc, LKP_ALPHA2), h1_x - h2_nx), lkp_scalar<9, P>(s_sc, LKP_ALPHA3), z_m1));
    // reduce_with_powers over [z1, shift, hs, last] (plonk_util.rs:27-33): three products through one reduction
    const auto res = lz_reduce(lz_mac(lz_mac(lz_mac(lz_wide<P>(), lz_table<P>(l0_tab, i), z_m1), lkp_scalar<16, P>(s_sc, LKP_ALPHA), shift),
                                      lz_table<P>(l0_tab, next), tail));
    fe_store<P>(out + i * 2, lz_to_rform<P>(res));
}

template <class P>
static int lookup_points_t(unsigned log_size, const void* d_values, const LookupScalars& sc, void* d_out, hipStream_t stream) {
    std::shared_ptr<LookupTables> tb;
    PLK_TRY(get_lookup_tables<P>((int)log_size, stream, tb));
    const size_t n4 = (size_t)4 << log_size;
    ScratchSet ss(stream);
    uint32_t* scal = (uint32_t*)ss.get((size_t)LKP_SCALARS * FzCfg<P>::NZ * 4);
    if (!scal) return PLK_ERR_OOM;
    k_lookup_scalars<P><<<1, 64, 0, stream>>>(sc, (const uint4*)tb->xs_lo_z.p, (const uint4*)tb->xs_hi_z.p, n4 - 4, scal);
    k_lookup_points<P><<<(unsigned)((n4 + 127) / 128), 128, 0, stream>>>((const uint4*)d_values, (const uint4*)tb->xs_lo_z.p, (const uint4*)tb->xs_hi_z.p,
                                                                         (const uint4*)tb->l0.p, scal, (int)log_size, (uint4*)d_out, (const uint32_t*)tb->top.p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "plookup vanishing points launch failed: %s", hipGetErrorString(e));
    // the tables stay alive in the cache (plk_ntt_clear_cache / plk_shutdown drop them after a device synchronisation)
    return PLK_OK;
}

int plookup_vanishing_points_dev_impl(unsigned log_size, int field, const void* d_values_4n, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma,
                                      void* d_out, hipStream_t stream) {
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a circuit scalar field", field);
    if (log_size == 0) return set_error(PLK_ERR_INVALID_ARG, "log_size 0: the prover pads to n + 1 >= 2 rows");
    if (log_size + 2 > 30) return set_error(PLK_ERR_TWO_ADICITY, "log_size %u too large", log_size);
    if (!d_values_4n || !d_out) return set_error(PLK_ERR_INVALID_ARG, "null device pointer");
    if (!alpha || !beta || !gamma) return set_error(PLK_ERR_INVALID_ARG, "null challenge pointer");
    PLK_TRY(ensure_device());
    LookupScalars sc;
    fill_lookup_scalars(sc, alpha, beta, gamma);
    return or_invalid(with_field4(field, [&](auto t) { return lookup_points_t<tag_t<decltype(t)>>(log_size, d_values_4n, sc, d_out, stream); }),
                      "field %d is not a circuit scalar field", field);
}

}  // namespace plk
