// opening.hip -- the opening step of the prover between the commitments and the inner-product argument:
//   * open_all_polynomials (plonk.rs:261-284, 459-482): every polynomial at every opening point (eval_polys / eval_from_power);
//   * the preamble of batch_opening_proof (halo.rs:38-44): reduced_coeffs[j] = sum_i s_i c_i[j], the argument's halo_a;
//   * build_halo_b (halo.rs:143-155), powers (plonk_util.rs:123-133) and halo_s (plonk_util.rs:311-326).
// Everything is exact field arithmetic on fully reduced results: any summation order gives the reference's words.
//
// Forms.  Coefficients are the reference's R-form words (value c 2^256, canonical).  Every multiplier TABLE holds canonical
// R'-form values (x 2^261, tables.cuh: to_rprime), so a product of a coefficient and a table entry on 29-bit limbs (fz.cuh) is
// R-form again.  Sums of products go through the column accumulators (FzWide): up to OPEN_GROUP = 6 products of exactly
// normalised operands (limbs < 2^29: a loaded word re-sliced, a table entry) share ONE Montgomery reduction - the column bound of
// fz.cuh (FZ_WIDE_UNITS) - and come back below 6 p p / R' + p < 1.1 p.
//
// Evaluation.  A workgroup of 256 lanes owns a tile of OPEN_TILE = 256 * 24 coefficients of one polynomial; lane l reads the
// coefficients tile + 256 m + l, m < 24 (consecutive lanes read consecutive elements: every load of a wave is one contiguous 2 KiB),
// in 4 rows of 6.  Per row and point it forms sum_t c_t (x^256)^(6 r + t) with one reduction; the powers (x^256)^m are the same for
// every lane (a table of 24 entries per point, read through wave-uniform loads), so no power vector exists anywhere.  The lane's sum is
// multiplied by x^l (a table of 256 entries per point), the workgroup adds its lanes up, and a second small launch adds the tiles of a
// (polynomial, point) with their x^(tile OPEN_TILE).  Each coefficient is read from HBM once, for all points.
#include <utility>
#include <vector>

#include "common.h"
#include "fp.cuh"
#include "fz.cuh"
#include "tables.cuh"

namespace plk {

constexpr int OPEN_LANES = 256;
constexpr int OPEN_GROUP = 6;   // products per reduction (FZ_WIDE_UNITS)
constexpr int OPEN_ROWS = 4;    // rows of OPEN_GROUP coefficients per lane and tile
constexpr int OPEN_PER_LANE = OPEN_GROUP * OPEN_ROWS;
constexpr size_t OPEN_TILE = (size_t)OPEN_LANES * OPEN_PER_LANE;  // 6144 coefficients
constexpr int OPEN_MAX_POINTS = 8;
constexpr int OPEN_CHUNK = 56;  // polynomials described per launch of k_open_describe (kernel arguments: 56 * 64 B + the rest < 4 KiB)
constexpr int OPEN_LO_LOG = 10; // two-level tables of the generated vectors: element j = lo[j & 1023] * hi[j >> 10]
constexpr size_t OPEN_LO = (size_t)1 << OPEN_LO_LOG;
constexpr unsigned OPEN_MAX_US = 30;
static_assert(OPEN_GROUP <= FZ_WIDE_UNITS, "column bound of the shared reduction");

// what the kernels know about the polynomials of a call, in device memory (written by k_open_describe from kernel arguments:
// no host buffer has to outlive the call, nothing is copied)
struct OpenDesc {
    const uint4** ptr;   // [n_polys]
    uint64_t* len;       // [n_polys]
    uint64_t* tile_off;  // [n_polys] tiles of the polynomials before this one (evaluation)
    uint32_t* scalar;    // [n_polys] limb form, R'-form (reduction)
};
struct OpenChunk {
    const void* ptr[OPEN_CHUNK];
    uint64_t len[OPEN_CHUNK];
    uint64_t tile_off[OPEN_CHUNK];
    uint32_t scalar[OPEN_CHUNK][8];
};
struct OpenPoints {
    uint32_t x[OPEN_MAX_POINTS][8];
    uint32_t v[8];
};
struct OpenUs {
    uint32_t u[OPEN_MAX_US][8];
};

template <class P> __global__ void __launch_bounds__(64) k_open_describe(OpenChunk c, unsigned first, unsigned count, int with_scalars, OpenDesc d) {
    const unsigned i = threadIdx.x;
    if (i >= count) return;
    d.ptr[first + i] = (const uint4*)c.ptr[i];
    d.len[first + i] = c.len[i];
    d.tile_off[first + i] = c.tile_off[i];
    if (with_scalars) limbs_store<P>(d.scalar, first + i, fz_from_fe<P>(to_rprime<P>(fe_from_words<P>(c.scalar[i]))));
}

// per point k: ytab[k][m] = x^(256 m), m < 24 (limb form), ltab[k][l] = x^l, l < 256 (words) - both R'-form - and xtile[k] = x^OPEN_TILE (R-form)
template <class P>
__global__ void __launch_bounds__(OPEN_LANES) k_open_tables(OpenPoints pts, uint32_t* __restrict__ ytab, uint4* __restrict__ ltab, uint4* __restrict__ xtile) {
    const int k = blockIdx.x, l = threadIdx.x;
    const Fe<P> x = fe_from_words<P>(pts.x[k]);
    fe_store<P>(ltab + ((size_t)k * OPEN_LANES + l) * (P::NL / 4), to_rprime<P>(fe_pow_u64<P>(x, (uint64_t)l)));
    if (l < OPEN_PER_LANE) limbs_store<P>(ytab, (size_t)k * OPEN_PER_LANE + l, fz_from_fe<P>(to_rprime<P>(fe_pow_u64<P>(x, (uint64_t)OPEN_LANES * l))));
    if (l == OPEN_PER_LANE) fe_store<P>(xtile + k * (P::NL / 4), fe_pow_u64<P>(x, (uint64_t)OPEN_TILE));
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): the per-point accumulators stay in registers only with constant indices
template <class F, int... I> PLK_DI void open_static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F> PLK_DI void open_static_for(F&& f) { open_static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// a table entry every lane of the wave reads alike: kept in scalar registers, where the multiplier takes it from
template <class P> PLK_DI Fz<P> limbs_load_uniform(const uint32_t* __restrict__ base, size_t e) {
    Fz<P> r = limbs_load<P>(base, e);
#pragma unroll
    for (int i = 0; i < FzCfg<P>::NZ; ++i) r.l[i] = __builtin_amdgcn_readfirstlane(r.l[i]);
    return r;
}

// sum of the 256 lanes' canonical values, through LDS; the result is valid on lane 0
template <class P> PLK_DI Fe<P> open_block_sum(Fe<P> acc, uint4* s_acc) {
    constexpr int W = P::NL / 4;
    __syncthreads();  // the previous user of s_acc has finished reading
    fe_store<P>(s_acc + threadIdx.x * W, acc);
    __syncthreads();
    for (int d = OPEN_LANES / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) {
            acc = fe_add<P>(acc, fe_load<P>(s_acc + (threadIdx.x + d) * W));
            fe_store<P>(s_acc + threadIdx.x * W, acc);
        }
        __syncthreads();
    }
    return acc;
}

// blockIdx.y: polynomial (from poly0), blockIdx.x: tile.  part[(tile_off[poly] + tile) * np + k] = sum over the tile of c_j x_k^(j - tile start), R-form
template <class P, int NPMAX>
__global__ void __launch_bounds__(OPEN_LANES) k_open_eval(OpenDesc d, unsigned poly0, int np, const uint32_t* __restrict__ ytab, const uint4* __restrict__ ltab,
                                                          uint4* __restrict__ part) {
    constexpr int W = P::NL / 4;
    __shared__ uint4 s_acc[OPEN_LANES * W];
    const unsigned poly = poly0 + blockIdx.y;
    const size_t len = d.len[poly], start = (size_t)blockIdx.x * OPEN_TILE;
    if (start >= len) return;
    const uint4* __restrict__ c = d.ptr[poly];
    Fz<P> acc[NPMAX];
    open_static_for<NPMAX>([&](auto K) { acc[K.value] = fz_zero<P>(); });
#pragma unroll 1
    for (int r = 0; r < OPEN_ROWS; ++r) {
        const size_t row = start + (size_t)r * OPEN_GROUP * OPEN_LANES;
        if (row < len) {
            Fz<P> cf[OPEN_GROUP];
#pragma unroll
            for (int t = 0; t < OPEN_GROUP; ++t) {
                const size_t j = row + (size_t)t * OPEN_LANES + threadIdx.x;
                cf[t] = j < len ? fz_from_fe<P>(fe_load<P>(c + j * W)) : fz_zero<P>();
            }
            open_static_for<NPMAX>([&](auto K) {
                constexpr int k = K.value;
                if (k < np) {
                    FzWide<P> w;
                    fz_wide_clear<P>(w);
#pragma unroll
                    for (int t = 0; t < OPEN_GROUP; ++t) fz_wide_mac<P>(w, cf[t], limbs_load_uniform<P>(ytab, (size_t)k * OPEN_PER_LANE + r * OPEN_GROUP + t));
                    acc[k] = fz_add<P>(acc[k], fz_wide_reduce<P>(w));  // below 1.1 p per row: below 4.4 p, limbs < 2^29 + 8
                }
            });
        }
    }
    open_static_for<NPMAX>([&](auto K) {
        constexpr int k = K.value;
        if (k < np) {
            const Fz<P> xl = fz_from_fe<P>(fe_load<P>(ltab + ((size_t)k * OPEN_LANES + threadIdx.x) * W));
            const Fe<P> sum = open_block_sum<P>(fz_to_fe_canonical<P>(fz_mul<P>(acc[k], xl)), s_acc);
            if (threadIdx.x == 0) fe_store<P>(part + ((d.tile_off[poly] + blockIdx.x) * (size_t)np + k) * W, sum);
        }
    });
}

// blockIdx.x = poly * np + k: out[k * n_polys + poly] = sum_tile part[tile] x_k^(tile OPEN_TILE)
template <class P>
__global__ void __launch_bounds__(OPEN_LANES) k_open_combine(OpenDesc d, unsigned n_polys, int np, const uint4* __restrict__ xtile, const uint4* __restrict__ part,
                                                             uint4* __restrict__ out) {
    constexpr int W = P::NL / 4;
    __shared__ uint4 s_acc[OPEN_LANES * W];
    const unsigned poly = blockIdx.x / (unsigned)np;
    const int k = (int)(blockIdx.x % (unsigned)np);
    const size_t tiles = (d.len[poly] + OPEN_TILE - 1) / OPEN_TILE, off = d.tile_off[poly];
    Fe<P> acc = fe_zero<P>();
    if (threadIdx.x < tiles) {
        const Fe<P> x = fe_load<P>(xtile + k * W);
        Fe<P> pw = fe_pow_u64<P>(x, (uint64_t)threadIdx.x);
        const Fe<P> step = tiles > OPEN_LANES ? fe_pow_u64<P>(x, (uint64_t)OPEN_LANES) : fe_one<P>();
        for (size_t t = threadIdx.x; t < tiles; t += OPEN_LANES) {
            acc = fe_add<P>(acc, fe_mul<P>(fe_load<P>(part + ((off + t) * (size_t)np + k) * W), pw));
            pw = fe_mul<P>(pw, step);
        }
    }
    acc = open_block_sum<P>(acc, s_acc);
    if (threadIdx.x == 0) fe_store<P>(out + ((size_t)k * n_polys + poly) * W, acc);
}

// out[j] = sum_i s_i c_i[j], j < degree; polynomials shorter than degree count as zero-padded
template <class P>
__global__ void __launch_bounds__(OPEN_LANES) k_poly_reduce(OpenDesc d, unsigned n_polys, size_t degree, uint4* __restrict__ out) {
    constexpr int W = P::NL / 4;
    const size_t first = (size_t)blockIdx.x * OPEN_LANES, j = first + threadIdx.x;
    Fz<P> total = fz_zero<P>();
    int groups = 0;
    for (unsigned i0 = 0; i0 < n_polys; i0 += OPEN_GROUP) {
        FzWide<P> w;
        fz_wide_clear<P>(w);
        bool any = false;
#pragma unroll
        for (int t = 0; t < OPEN_GROUP; ++t) {
            const unsigned i = i0 + t;
            if (i < n_polys && first < d.len[i]) {  // uniform: the workgroup's first element
                const uint4* __restrict__ c = d.ptr[i];
                const Fz<P> cf = j < d.len[i] ? fz_from_fe<P>(fe_load<P>(c + j * W)) : fz_zero<P>();
                fz_wide_mac<P>(w, cf, limbs_load<P>(d.scalar, i));
                any = true;
            }
        }
        if (!any) continue;
        total = fz_add<P>(total, fz_wide_reduce<P>(w));  // + less than 1.1 p
        if (++groups == 5) {                             // below 6.6 p < R' / 8: bring it back below 1.1 p
            total = fz_mul<P>(total, fz_one_rprime<P>());
            groups = 0;
        }
    }
    if (j < degree) fe_store<P>(out + j * W, fz_to_fe_canonical<P>(fz_mul<P>(total, fz_one_rprime<P>())));
}

// ---- the generated vectors: powers, halo_b, halo_s: out[j] = sum_k lo[k][j & 1023] hi[k][j >> 10] ----
// lo[k][a] = x_k^a (R-form), hi[k][b] = v^k x_k^(1024 b) (R'-form), b < nhi
template <class P>
__global__ void __launch_bounds__(OPEN_LANES) k_open_pow_tables(OpenPoints pts, int np, size_t nhi, uint4* __restrict__ lo, uint4* __restrict__ hi) {
    constexpr int W = P::NL / 4;
    const size_t per = OPEN_LO + nhi, i = (size_t)blockIdx.x * OPEN_LANES + threadIdx.x;
    if (i >= per * (size_t)np) return;
    const int k = (int)(i / per);
    const size_t e = i % per;
    const Fe<P> x = fe_from_words<P>(pts.x[k]);
    if (e < OPEN_LO) {
        fe_store<P>(lo + ((size_t)k * OPEN_LO + e) * W, fe_pow_u64<P>(x, e));
    } else {
        Fe<P> y = x;
        for (int s = 0; s < OPEN_LO_LOG; ++s) y = fe_sqr<P>(y);
        const Fe<P> vk = fe_pow_u64<P>(fe_from_words<P>(pts.v), (uint64_t)k);
        fe_store<P>(hi + ((size_t)k * nhi + (e - OPEN_LO)) * W, to_rprime<P>(fe_mul<P>(vk, fe_pow_u64<P>(y, e - OPEN_LO))));
    }
}
// halo_s (plonk_util.rs:311-326): element i = prod_j (bit j of i ? u : 1 / u)[k - 1 - j].  The k inversions are one lane each of a launch
// of their own (uinv); lo[a]: the factors of bits 0..9, hi[b]: the others
template <class P> __global__ void __launch_bounds__(64) k_halo_s_inverses(OpenUs us, unsigned k, uint4* __restrict__ uinv) {
    if (threadIdx.x < k) fe_store<P>(uinv + threadIdx.x * (P::NL / 4), fe_inv_safegcd<P>(fe_from_words<P>(us.u[threadIdx.x])));
}
template <class P>
__global__ void __launch_bounds__(OPEN_LANES) k_halo_s_tables(OpenUs us, const uint4* __restrict__ uinv, unsigned k, size_t nlo, size_t nhi, uint4* __restrict__ lo,
                                                              uint4* __restrict__ hi) {
    constexpr int W = P::NL / 4;
    const size_t i = (size_t)blockIdx.x * OPEN_LANES + threadIdx.x;
    if (i >= nlo + nhi) return;
    const bool low = i < nlo;
    const size_t bits = low ? i : i - nlo;
    const unsigned j0 = low ? 0u : (unsigned)OPEN_LO_LOG, j1 = low ? (k < (unsigned)OPEN_LO_LOG ? k : (unsigned)OPEN_LO_LOG) : k;
    Fe<P> r = fe_one<P>();
    for (unsigned j = j0; j < j1; ++j) {
        const unsigned idx = k - 1 - j;
        r = fe_mul<P>(r, ((bits >> (j - j0)) & 1) ? fe_from_words<P>(us.u[idx]) : fe_load<P>(uinv + idx * W));
    }
    if (low) fe_store<P>(lo + i * W, r);
    else fe_store<P>(hi + (i - nlo) * W, to_rprime<P>(r));
}
template <class P>
__global__ void __launch_bounds__(OPEN_LANES) k_open_two_level(const uint4* __restrict__ lo, const uint4* __restrict__ hi, int np, size_t nlo, size_t nhi, size_t count,
                                                               uint4* __restrict__ out) {
    constexpr int W = P::NL / 4;
    const size_t j = (size_t)blockIdx.x * OPEN_LANES + threadIdx.x;
    if (j >= count) return;
    const size_t a = j & (OPEN_LO - 1), b = j >> OPEN_LO_LOG;
    Fe<P> res = fe_zero<P>();
    for (int k0 = 0; k0 < np; k0 += OPEN_GROUP) {
        FzWide<P> w;
        fz_wide_clear<P>(w);
        for (int k = k0; k < np && k < k0 + OPEN_GROUP; ++k)
            fz_wide_mac<P>(w, fz_from_fe<P>(fe_load<P>(lo + ((size_t)k * nlo + a) * W)), fz_from_fe<P>(fe_load<P>(hi + ((size_t)k * nhi + b) * W)));
        const Fe<P> s = fz_to_fe_canonical<P>(fz_wide_reduce<P>(w));
        res = k0 == 0 ? s : fe_add<P>(res, s);
    }
    fe_store<P>(out + j * W, res);
}

// ---- host side ----
static int check_polys(unsigned n_polys, const void* const* d_polys, const size_t* lens) {
    if (n_polys && (!d_polys || !lens)) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    for (unsigned i = 0; i < n_polys; ++i)
        if (lens[i] && !d_polys[i]) return set_error(PLK_ERR_INVALID_ARG, "null pointer: polynomial %u", i);
    return PLK_OK;
}

// the descriptors of the call, written to device memory by launches that carry them as kernel arguments
template <class P>
static int describe(ScratchSet& ss, unsigned n_polys, const void* const* d_polys, const size_t* lens, const uint64_t* scalars, OpenDesc& d, size_t* total_tiles) {
    const size_t n = n_polys ? n_polys : 1;
    d.ptr = (const uint4**)ss.get(n * sizeof(void*));
    d.len = (uint64_t*)ss.get(n * sizeof(uint64_t));
    d.tile_off = (uint64_t*)ss.get(n * sizeof(uint64_t));
    d.scalar = (uint32_t*)ss.get(limb_bytes(n, FzCfg<P>::NZ));
    if (!d.ptr || !d.len || !d.tile_off || !d.scalar) return PLK_ERR_OOM;  // scratch_acquire has set the error text
    size_t tiles = 0;
    for (unsigned first = 0; first < n_polys; first += OPEN_CHUNK) {
        OpenChunk c = {};
        const unsigned count = n_polys - first < (unsigned)OPEN_CHUNK ? n_polys - first : (unsigned)OPEN_CHUNK;
        for (unsigned i = 0; i < count; ++i) {
            c.ptr[i] = d_polys[first + i];
            c.len[i] = lens[first + i];
            c.tile_off[i] = tiles;
            tiles += (lens[first + i] + OPEN_TILE - 1) / OPEN_TILE;
            if (scalars) limbs_to_words(c.scalar[i], scalars + (size_t)(first + i) * 4);
        }
        k_open_describe<P><<<1, 64, 0, ss.stream>>>(c, first, count, scalars ? 1 : 0, d);
    }
    if (total_tiles) *total_tiles = tiles;
    return PLK_OK;
}

template <class P>
static int eval_polys_t(unsigned n_polys, const void* const* d_polys, const size_t* lens, unsigned n_points, const uint64_t* points, void* d_out, hipStream_t stream) {
    ScratchSet ss(stream);
    OpenDesc d;
    size_t tiles = 0, max_len = 0;
    for (unsigned i = 0; i < n_polys; ++i) max_len = lens[i] > max_len ? lens[i] : max_len;
    PLK_TRY(describe<P>(ss, n_polys, d_polys, lens, nullptr, d, &tiles));
    uint32_t* ytab = (uint32_t*)ss.get(limb_bytes((size_t)n_points * OPEN_PER_LANE, FzCfg<P>::NZ));
    uint4* ltab = (uint4*)ss.get((size_t)n_points * OPEN_LANES * 32);
    uint4* xtile = (uint4*)ss.get((size_t)n_points * 32);
    uint4* part = (uint4*)ss.get(tiles * n_points * 32);
    if (!ytab || !ltab || !xtile || !part) return PLK_ERR_OOM;
    OpenPoints pts = {};
    for (unsigned k = 0; k < n_points; ++k) limbs_to_words(pts.x[k], points + (size_t)k * 4);
    k_open_tables<P><<<n_points, OPEN_LANES, 0, stream>>>(pts, ytab, ltab, xtile);
    const size_t max_tiles = (max_len + OPEN_TILE - 1) / OPEN_TILE;
    for (unsigned poly0 = 0; poly0 < n_polys && max_tiles; poly0 += 32768u) {
        const dim3 grid((unsigned)max_tiles, n_polys - poly0 < 32768u ? n_polys - poly0 : 32768u);
        if (n_points == 1) k_open_eval<P, 1><<<grid, OPEN_LANES, 0, stream>>>(d, poly0, (int)n_points, ytab, ltab, part);
        else if (n_points <= 3) k_open_eval<P, 3><<<grid, OPEN_LANES, 0, stream>>>(d, poly0, (int)n_points, ytab, ltab, part);
        else k_open_eval<P, OPEN_MAX_POINTS><<<grid, OPEN_LANES, 0, stream>>>(d, poly0, (int)n_points, ytab, ltab, part);
    }
    k_open_combine<P><<<n_polys * n_points, OPEN_LANES, 0, stream>>>(d, n_polys, (int)n_points, xtile, part, (uint4*)d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "polynomial evaluation launch (descriptors, tables, tiles or combine) failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

template <class P>
static int poly_reduce_t(unsigned n_polys, const void* const* d_polys, const size_t* lens, const uint64_t* scalars, size_t degree, void* d_out, hipStream_t stream) {
    ScratchSet ss(stream);
    OpenDesc d;
    PLK_TRY(describe<P>(ss, n_polys, d_polys, lens, scalars, d, nullptr));
    k_poly_reduce<P><<<(unsigned)((degree + OPEN_LANES - 1) / OPEN_LANES), OPEN_LANES, 0, stream>>>(d, n_polys, degree, (uint4*)d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "polynomial reduction launch (descriptors or reduction) failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

template <class P> static int build_b_t(unsigned n_points, const uint64_t* points, const uint64_t* v, size_t degree, void* d_out, hipStream_t stream) {
    ScratchSet ss(stream);
    const size_t nhi = (degree + OPEN_LO - 1) >> OPEN_LO_LOG;
    uint4* lo = (uint4*)ss.get((size_t)n_points * OPEN_LO * 32);
    uint4* hi = (uint4*)ss.get((size_t)n_points * nhi * 32);
    if (!lo || !hi) return PLK_ERR_OOM;
    OpenPoints pts = {};
    for (unsigned k = 0; k < n_points; ++k) limbs_to_words(pts.x[k], points + (size_t)k * 4);
    limbs_to_words(pts.v, v);
    const size_t lanes = (OPEN_LO + nhi) * n_points;
    k_open_pow_tables<P><<<(unsigned)((lanes + OPEN_LANES - 1) / OPEN_LANES), OPEN_LANES, 0, stream>>>(pts, (int)n_points, nhi, lo, hi);
    k_open_two_level<P><<<(unsigned)((degree + OPEN_LANES - 1) / OPEN_LANES), OPEN_LANES, 0, stream>>>(lo, hi, (int)n_points, OPEN_LO, nhi, degree, (uint4*)d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "power vector launch (tables or the two-level product) failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

template <class P> static int halo_s_t(unsigned k, const uint64_t* us, void* d_out, hipStream_t stream) {
    ScratchSet ss(stream);
    const size_t n = (size_t)1 << k, nlo = n < OPEN_LO ? n : OPEN_LO, nhi = n >> (k < (unsigned)OPEN_LO_LOG ? k : (unsigned)OPEN_LO_LOG);
    uint4* lo = (uint4*)ss.get(nlo * 32);
    uint4* hi = (uint4*)ss.get(nhi * 32);
    uint4* uinv = (uint4*)ss.get((size_t)OPEN_MAX_US * 32);
    if (!lo || !hi || !uinv) return PLK_ERR_OOM;  // scratch_acquire has set the error text
    OpenUs arg = {};
    for (unsigned j = 0; j < k; ++j) limbs_to_words(arg.u[j], us + (size_t)j * 4);
    k_halo_s_inverses<P><<<1, 64, 0, stream>>>(arg, k, uinv);
    k_halo_s_tables<P><<<(unsigned)((nlo + nhi + OPEN_LANES - 1) / OPEN_LANES), OPEN_LANES, 0, stream>>>(arg, uinv, k, nlo, nhi, lo, hi);
    // element i = lo[i & 1023] hi[i >> 10]: nlo = 2^k below 2^10 elements, where i >> 10 = 0 and i & 1023 = i
    k_open_two_level<P><<<(unsigned)((n + OPEN_LANES - 1) / OPEN_LANES), OPEN_LANES, 0, stream>>>(lo, hi, 1, nlo, nhi, n, (uint4*)d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PLK_ERR_HIP, "halo_s launch (inverses, tables or the two-level product) failed: %s", hipGetErrorString(e));
    return PLK_OK;
}

// dispatch of the entry points below: every one has passed check_field, which gives the id's error first, as the callers expect
template <class F> static int open_dispatch(int field, F&& f) { return or_invalid(with_field4(field, f), "field %d is not a 4-limb field", field); }

static int check_field(int field) {
    if (field_limbs(field) != 4) return set_error(PLK_ERR_INVALID_ARG, "field %d is not a 4-limb field", field);
    return PLK_OK;
}

int plonk_eval_polys_dev_impl(int field, unsigned n_polys, const void* const* d_polys, const size_t* lens, unsigned n_points, const uint64_t* points, void* d_out,
                              hipStream_t stream) {
    PLK_TRY(check_field(field));
    if (n_points < 1 || n_points > (unsigned)OPEN_MAX_POINTS) return set_error(PLK_ERR_INVALID_ARG, "n_points %u is not in 1..%d", n_points, OPEN_MAX_POINTS);
    if (!points) return set_error(PLK_ERR_INVALID_ARG, "null pointer: points");
    PLK_TRY(check_polys(n_polys, d_polys, lens));
    if (n_polys == 0) return PLK_OK;
    if (!d_out) return set_error(PLK_ERR_INVALID_ARG, "null pointer: output");
    PLK_TRY(ensure_device());
    return open_dispatch(field, [&](auto t) { return eval_polys_t<tag_t<decltype(t)>>(n_polys, d_polys, lens, n_points, points, d_out, stream); });
}

int poly_reduce_dev_impl(int field, unsigned n_polys, const void* const* d_polys, const size_t* lens, const uint64_t* scalars, size_t degree, void* d_out,
                         hipStream_t stream) {
    PLK_TRY(check_field(field));
    PLK_TRY(check_polys(n_polys, d_polys, lens));
    if (n_polys && !scalars) return set_error(PLK_ERR_INVALID_ARG, "null pointer: scalars");
    for (unsigned i = 0; i < n_polys; ++i)
        if (lens[i] > degree) return set_error(PLK_ERR_INVALID_ARG, "polynomial %u has %zu coefficients, more than the degree %zu (halo.rs:41)", i, lens[i], degree);
    if (degree == 0) return PLK_OK;
    if (!d_out) return set_error(PLK_ERR_INVALID_ARG, "null pointer: output");
    PLK_TRY(ensure_device());
    return open_dispatch(field, [&](auto t) { return poly_reduce_t<tag_t<decltype(t)>>(n_polys, d_polys, lens, scalars, degree, d_out, stream); });
}

int halo_build_b_dev_impl(int field, unsigned n_points, const uint64_t* points, const uint64_t* v, size_t degree, void* d_out, hipStream_t stream) {
    PLK_TRY(check_field(field));
    if (n_points < 1 || n_points > (unsigned)OPEN_MAX_POINTS) return set_error(PLK_ERR_INVALID_ARG, "n_points %u is not in 1..%d", n_points, OPEN_MAX_POINTS);
    if (!points || !v) return set_error(PLK_ERR_INVALID_ARG, "null pointer: points / v");
    if (degree == 0) return PLK_OK;
    if (!d_out) return set_error(PLK_ERR_INVALID_ARG, "null pointer: output");
    PLK_TRY(ensure_device());
    return open_dispatch(field, [&](auto t) { return build_b_t<tag_t<decltype(t)>>(n_points, points, v, degree, d_out, stream); });
}

int halo_s_dev_impl(int field, unsigned k, const uint64_t* us, void* d_out, hipStream_t stream) {
    PLK_TRY(check_field(field));
    if (k > OPEN_MAX_US) return set_error(PLK_ERR_INVALID_ARG, "%u challenges: at most %u", k, OPEN_MAX_US);
    if ((k && !us) || !d_out) return set_error(PLK_ERR_INVALID_ARG, "null pointer");
    for (unsigned j = 0; j < k; ++j)
        if (!(us[4 * j] | us[4 * j + 1] | us[4 * j + 2] | us[4 * j + 3]))
            return set_error(PLK_ERR_INVALID_ARG, "No inverse: challenge %u is zero (field.rs:266, from plonk_util.rs:314)", j);
    PLK_TRY(ensure_device());
    return open_dispatch(field, [&](auto t) { return halo_s_t<tag_t<decltype(t)>>(k, us, d_out, stream); });
}

}  // namespace plk
