// GF(2^64) on gfx950: the protocol-layer steps of the encoded Aurora prover — the one-word twins of encoded_ops.hip / virtual_oracles.hip.
//
//   iopx_gf64_add_dev, iopx_gf64_pow_table_dev     elementwise helpers, the powers of alpha (basic_lincheck_aux.tcc:37-45)
//   iopx_lincomb{,_affine}_gf64_dev                random_linear_combination_oracle::evaluated_contents (random_linear_combination.tcc:27-57),
//                                                  single_matrix_denominator::evaluated_contents (holographic_lincheck_aux.tcc:117-143)
//   iopx_spmv_gf64_dev                             create_Az_Bz_Cz_from_variable_assignment (r1cs.tcc:236-268), p_alpha_ABC (basic_lincheck_aux.tcc:64-88)
//   iopx_lincheck_gf64_dev                         multi_lincheck_virtual_oracle::evaluated_contents (basic_lincheck_aux.tcc:102-144)
//   iopx_rowcheck_gf64_dev                         rowcheck_ABC_virtual_oracle::evaluated_contents (rowcheck.tcc:16-88)
//   iopx_fz_gf64_dev                               fz_virtual_oracle::evaluated_contents (r1cs_rs_iop.tcc:181-222)
//   iopx_sumcheck_g_gf64_dev                       sumcheck_g_oracle::evaluated_contents (sumcheck.tcc:58-119)
//   iopx_poly_div_vanishing_gf64_dev               polynomial_over_vanishing_polynomial(...).first (vanishing_polynomial.tcc:314-371)
//   iopx_div_by_vanishing_gf64_dev,                the head route's pointwise division by Z_S and the host's Z_S(x) (include/libiop_amd_head.h)
//   iopx_gf64_vanishing_host
//
// An element is 8 bytes and a product ~0.13k VALU ops (gf64_dev.h): every kernel here is bound by its HBM passes, so each one reads every
// input once and writes the output once, in a grid-stride loop.  Where the position of an element does not enter the addressing beyond
// "j and j + 1" a lane takes two consecutive elements with one 16-byte access (V = 2; chosen on the host when every vector is 16-byte
// aligned, V = 1 otherwise); the CSR gather and the division passes (odd offsets) take one.  Constants of a launch (coefficients, the
// squares of a base, the terms of a division pass) travel in the kernel's argument block: no upload, no wave-uniform multiplier form.
// The domain-shaped values Z_I(x_j), Z_H(x_j), x_j, x_j^|H| are subset sums of an (m + 1)-entry table over the bits of j
// (linearized_polynomial.tcc:83-108); position j + 1 of a pair differs from position j by the table's entry for bit 0.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "gf64_dev.h"
#include "gf64_host.h"
#include "runtime.h"

namespace iopx {

struct alignas(16) u64x2 { uint64_t a, b; };

static int ops64_grid(size_t work)
{
    size_t g = (work + 255) / 256;
    if (g > 16384) g = 16384;
    return (int)(g ? g : 1);
}

// ... under the option IOPX_GF64_OPS_MAX_BLOCKS (default: the cap above; looked up per launch; a test helper as gfx_ops.h's IOPX_GFX_OPS_MAX_BLOCKS:
// a small cap sends a grid-stride loop round again at a few thousand elements)
static int ops64_grid_capped(size_t work)
{
    const int g = ops64_grid(work), cap = opt_range("IOPX_GF64_OPS_MAX_BLOCKS", 16384, 1, 16384);
    return g < cap ? g : cap;
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ uint64_t mul64(uint64_t a, uint64_t b)
{
    return g64_word(g64_mul(g64_from(a), g64_from(b)));
}

// elements [j, j + V) of a vector of n; with V = 2, j is even and the second element of the last pair of an odd n is absent
template<int V>
__device__ __forceinline__ void ld64(uint64_t (&v)[V], const uint64_t *p, size_t j, size_t n)
{
    if constexpr (V == 2) {
        if (j + 1 < n) { const u64x2 t = *reinterpret_cast<const u64x2 *>(p + j); v[0] = t.a; v[1] = t.b; }
        else { v[0] = p[j]; v[1] = 0; }
    } else {
        v[0] = p[j];
    }
}

template<int V>
__device__ __forceinline__ void st64(uint64_t *p, size_t j, size_t n, const uint64_t (&v)[V])
{
    if constexpr (V == 2) {
        if (j + 1 < n) { u64x2 t; t.a = v[0]; t.b = v[1]; *reinterpret_cast<u64x2 *>(p + j) = t; }
        else p[j] = v[0];
    } else {
        p[j] = v[0];
    }
}

#define OPS64_LOOP(V, j, n) \
    for (size_t j = (size_t)(V) * ((size_t)blockIdx.x * blockDim.x + threadIdx.x); j < (n); j += (size_t)(V) * gridDim.x * blockDim.x)

// t[0] + sum_{bit k of j} t[1 + k], j < 2^m
__device__ __forceinline__ uint64_t subset_sum64(const uint64_t *t, int m, size_t j)
{
    uint64_t v = t[0];
    for (int k = 0; k < m; ++k) v ^= ((j >> k) & 1) ? t[1 + k] : 0;
    return v;
}

// the sums at positions j .. j + V - 1 (j even when V = 2; the second one is only used when j + 1 < 2^m, so m >= 1 there)
template<int V>
__device__ __forceinline__ void subset_sums64(uint64_t (&z)[V], const uint64_t *t, int m, size_t j)
{
    z[0] = subset_sum64(t, m, j);
    if constexpr (V == 2) z[1] = m > 0 ? z[0] ^ t[1] : 0;
}

// ---- elementwise ----------------------------------------------------------------------------------------------------------
template<int V>
__global__ void __launch_bounds__(256) k64_add(uint64_t *out, const uint64_t *a, const uint64_t *b, size_t n)
{
    OPS64_LOOP(V, j, n) {
        uint64_t x[V], y[V];
        ld64<V>(x, a, j, n); ld64<V>(y, b, j, n);
#pragma unroll
        for (int e = 0; e < V; ++e) x[e] ^= y[e];
        st64<V>(out, j, n, x);
    }
}

// out[l] = init * base^l: the product of sq[k] = base^(2^k) over the set bits of l
#define POW64_MAX_BITS 40
struct PowParams64 {
    uint64_t sq[POW64_MAX_BITS];
    uint64_t init;
    int nbits;
};

__global__ void __launch_bounds__(256) k64_pow_table(uint64_t *out, size_t count, PowParams64 p)
{
    for (size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x; l < count; l += (size_t)gridDim.x * blockDim.x) {
        gf64 acc = g64_from(p.init);
        for (int k = 0; k < p.nbits; ++k) {
            if ((l >> k) & 1) acc = g64_mul(acc, g64_from(p.sq[k]));
        }
        out[l] = g64_word(acc);
    }
}

// ---- random linear combination ---------------------------------------------------------------------------------------------
#define LINCOMB64_MAX 16
struct LincombParams64 {
    const uint64_t *o[LINCOMB64_MAX];
    uint64_t c[LINCOMB64_MAX];
    uint64_t constant;          // zero when there is none
    uint64_t *out;
    int num;
    size_t n;
};

template<int V>
__global__ void __launch_bounds__(256) k64_lincomb(LincombParams64 p)
{
    OPS64_LOOP(V, j, p.n) {
        uint64_t acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = p.constant;
        for (int i = 0; i < p.num; ++i) {
            uint64_t x[V];
            ld64<V>(x, p.o[i], j, p.n);
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] ^= mul64(x[e], p.c[i]);
        }
        st64<V>(p.out, j, p.n, acc);
    }
}

// ---- CSR sparse matrix x vector: one lane per row ----------------------------------------------------------------------------
struct SpmvParams64 {
    const uint64_t *row_ptr;    // rows + 1 offsets
    const uint32_t *col;
    const uint64_t *coeff, *vec;
    uint64_t *out;
    uint64_t scale;
    size_t rows;
    int has_scale, accumulate;
};

__global__ void __launch_bounds__(256) k64_spmv(SpmvParams64 p)
{
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < p.rows; r += (size_t)gridDim.x * blockDim.x) {
        uint64_t acc = 0;
        const uint64_t e = p.row_ptr[r + 1];
        for (uint64_t t = p.row_ptr[r]; t < e; ++t) acc ^= mul64(p.vec[p.col[t]], p.coeff[t]);
        if (p.has_scale) acc = mul64(acc, p.scale);
        if (p.accumulate) acc ^= p.out[r];
        p.out[r] = acc;
    }
}

// ---- one factor (1 + u^(2^k)) of the power-series inverse (encoded_ops.hip) --------------------------------------------------
#define PDIV64_MAX_TERMS 66
struct PolyDivParams64 {
    const uint64_t *src;
    uint64_t *dst;
    uint64_t consts[PDIV64_MAX_TERMS];
    size_t off[PDIV64_MAX_TERMS];
    size_t M;
    int nterms;
};

__global__ void __launch_bounds__(256) k64_polydiv_pass(PolyDivParams64 p)
{
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.M; j += (size_t)gridDim.x * blockDim.x) {
        uint64_t acc = p.src[j];
        for (int t = 0; t < p.nterms; ++t) {
            const size_t s = j + p.off[t];
            if (s < p.M) acc ^= mul64(p.src[s], p.consts[t]);
        }
        p.dst[j] = acc;
    }
}

// ---- virtual oracles -----------------------------------------------------------------------------------------------------
// result[x] = (Az(x) Bz(x) - Cz(x)) / Z_H(x); cosets of H are the blocks position >> h of the codeword domain (virtual_oracles.hip)
template<int V>
__global__ void __launch_bounds__(256) k64_rowcheck(uint64_t *out, const uint64_t *az, const uint64_t *bz, const uint64_t *cz, const uint64_t *zinv, int h,
                                                    size_t n)
{
    OPS64_LOOP(V, j, n) {
        uint64_t a[V], b[V], c[V];
        ld64<V>(a, az, j, n); ld64<V>(b, bz, j, n); ld64<V>(c, cz, j, n);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if (j + e < n) a[e] = mul64(mul64(a[e], b[e]) ^ c[e], zinv[(j + e) >> h]);     // characteristic 2: a b - c = a b + c
        }
        st64<V>(out, j, n, a);
    }
}

// out[x] = in[x] / Z_S(x): Z_S is constant on the cosets of S, the blocks position >> s of the domain; one product per element, out may be in
template<int V>
__global__ void __launch_bounds__(256) k64_div_by_vanishing(uint64_t *out, const uint64_t *in, const uint64_t *zinv, int s, size_t n)
{
    OPS64_LOOP(V, j, n) {
        uint64_t a[V];
        ld64<V>(a, in, j, n);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if (j + e < n) a[e] = mul64(a[e], zinv[(j + e) >> s]);
        }
        st64<V>(out, j, n, a);
    }
}

// result[x] = fw(x) Z_I(x) + f_1v(x)
template<int V>
__global__ void __launch_bounds__(256) k64_fz(uint64_t *out, const uint64_t *fw, const uint64_t *f1v, const uint64_t *tab, int m, size_t n)
{
    OPS64_LOOP(V, j, n) {
        uint64_t w[V], f[V], z[V];
        ld64<V>(w, fw, j, n); ld64<V>(f, f1v, j, n);
        subset_sums64<V>(z, tab, m, j);
#pragma unroll
        for (int e = 0; e < V; ++e) w[e] = mul64(w[e], z[e]) ^ f[e];
        st64<V>(out, j, n, w);
    }
}

// p'(x) = f(x) - eps^-1 mu x^(|H| - 1) - Z_H(x) h(x), x^(|H| - 1) = x^|H| / x with 1 / 0 = 0 (sumcheck_aux.tcc:3-32, utils.tcc:79-97).
// NONZERO = false is the arm every shipped protocol takes (claimed sum 0: no middle term, no inversion).  The other arm inverts each
// x_j directly (Itoh-Tsujii, g64_inv maps 0 to 0): no staging in LDS and no per-lane batch, at 63 squarings + 10 products per element.
struct SumcheckParams64 {
    const uint64_t *f, *h;
    uint64_t *out;
    const uint64_t *xtab, *htab, *ztab;     // (m + 1)-entry subset-sum tables of x, x^|H|, Z_H(x)
    uint64_t c;                             // eps^-1 mu
    int m;
    size_t n;
};

template<int V, bool NONZERO>
__global__ void __launch_bounds__(256) k64_sumcheck_g(SumcheckParams64 p)
{
    OPS64_LOOP(V, j, p.n) {
        uint64_t f[V], h[V], z[V];
        ld64<V>(f, p.f, j, p.n); ld64<V>(h, p.h, j, p.n);
        subset_sums64<V>(z, p.ztab, p.m, j);
#pragma unroll
        for (int e = 0; e < V; ++e) f[e] ^= mul64(z[e], h[e]);
        if constexpr (NONZERO) {
            uint64_t x[V], xh[V];
            subset_sums64<V>(x, p.xtab, p.m, j);
            subset_sums64<V>(xh, p.htab, p.m, j);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const gf64 xinv_c = g64_mul(g64_inv(g64_from(x[e])), g64_from(p.c));
                f[e] ^= g64_word(g64_mul(g64_from(xh[e]), xinv_c));
            }
        }
        st64<V>(p.out, j, p.n, f);
    }
}

// result[x] = (sum_m r_m Mz_m(x)) p_alpha^1(x) - fz(x) p_alpha^2(x)
#define LINCHECK64_MAX_MATRICES 8
struct LincheckParams64 {
    const uint64_t *fz, *p1, *p2;
    const uint64_t *mz[LINCHECK64_MAX_MATRICES];
    uint64_t r[LINCHECK64_MAX_MATRICES];
    uint64_t *out;
    int num_matrices;
    size_t n;
};

template<int V>
__global__ void __launch_bounds__(256) k64_lincheck(LincheckParams64 p)
{
    OPS64_LOOP(V, j, p.n) {
        uint64_t comb[V], x[V], y[V];
#pragma unroll
        for (int e = 0; e < V; ++e) comb[e] = 0;
        for (int m = 0; m < p.num_matrices; ++m) {
            ld64<V>(x, p.mz[m], j, p.n);
#pragma unroll
            for (int e = 0; e < V; ++e) comb[e] ^= mul64(x[e], p.r[m]);
        }
        ld64<V>(x, p.p1, j, p.n);
#pragma unroll
        for (int e = 0; e < V; ++e) comb[e] = mul64(comb[e], x[e]);
        ld64<V>(x, p.fz, j, p.n); ld64<V>(y, p.p2, j, p.n);
#pragma unroll
        for (int e = 0; e < V; ++e) comb[e] ^= mul64(x[e], y[e]);
        st64<V>(p.out, j, p.n, comb);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static std::vector<hgf64> host_elems64(const uint64_t *w, size_t count)
{
    std::vector<hgf64> v(count);
    for (size_t i = 0; i < count; ++i) v[i] = hgf64(w[i]);
    return v;
}

// key of a table that depends on two gf64 domains: the tag keeps it apart from every gf192 table of runtime.hip's cache
static std::vector<uint64_t> table_key64(const uint64_t *basis, size_t m, const uint64_t *shift, const uint64_t *sub_basis, size_t sub_dim,
                                         const uint64_t *sub_shift, uint64_t tag)
{
    std::vector<uint64_t> key(basis, basis + m);
    key.push_back(shift[0]);
    if (sub_basis) key.insert(key.end(), sub_basis, sub_basis + sub_dim);
    key.push_back(sub_shift[0]);
    key.push_back(m); key.push_back(sub_dim); key.push_back(tag);
    return key;
}

// 1 / Z_H on each coset of H = span(basis[0..h)) + constraint_shift inside span(basis[0..m)) + shift (virtual_oracles.hip): evaluated on the
// host, inverted with Montgomery's trick (one field inversion), kept on the device per pair of domains and caller (`tag`; `meets`: the caller's
// refusal of a domain on which Z_H has a zero)
static int vanishing_inverse_table64(const uint64_t *basis, size_t m, const uint64_t *shift, size_t h, const uint64_t *constraint_shift, TmpBuf &dz,
                                     uint64_t tag = 0x3634726f77 /* "64row" */, const char *meets = "the codeword domain intersects the constraint domain")
{
    const size_t cosets = (size_t)1 << (m - h);
    return cached_domain_table(table_key64(basis, m, shift, nullptr, h, constraint_shift, tag), [&](std::vector<uint64_t> &zinv) -> int {
        const std::vector<hgf64> b = host_elems64(basis, m);
        const SubspacePoly64 lin(b.data(), h);
        const hgf64 z_shift = lin.eval(hgf64(constraint_shift[0]));
        std::vector<hgf64> z(cosets), prefix(cosets);
        hgf64 acc = hgf64::one();
        for (size_t c = 0; c < cosets; ++c) {
            hgf64 x(shift[0]);                                  // first element of the coset: index c << h (utils.tcc:8-30)
            for (size_t k = h; k < m; ++k) if ((c >> (k - h)) & 1) x += b[k];
            z[c] = lin.eval(x) + z_shift;
            if (z[c].is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "%s", meets);
            acc = acc * z[c];
            prefix[c] = acc;
        }
        hgf64 inv = acc.inverse();
        zinv.resize(cosets);
        for (size_t c = cosets; c-- > 0;) {
            zinv[c] = (c ? inv * prefix[c - 1] : inv).v;
            inv = inv * z[c];
        }
        return IOPX_OK;
    }, dz);
}

struct Term64 { size_t off; uint64_t c; };

// the passes of encoded_ops.hip's run_division on one-word elements
template<typename PassTerms>
static int run_division64(const uint64_t *d_high, size_t M, size_t min_offset, uint64_t *d_quotient, PassTerms terms_of_pass)
{
    int passes = 0;
    for (size_t o = min_offset; o != 0 && o < M; o <<= 1) ++passes;         // offsets stay below 2 M <= 2^41: no overflow
    if (passes == 0) return d_high != d_quotient ? copy_d2d(d_quotient, d_high, M * 8) : IOPX_OK;
    TmpBuf ping;
    int rc;
    if (passes > 1 && (rc = ping.alloc(M * 8)) != IOPX_OK) return rc;
    const uint64_t *src = d_high;
    for (int k = 0; k < passes; ++k) {
        // the last pass writes the quotient; before that alternate between the temporary and the quotient buffer
        uint64_t *dst = ((passes - 1 - k) & 1) ? ping.u64() : d_quotient;
        PolyDivParams64 p;
        memset(&p, 0, sizeof(p));
        for (const Term64 &t : terms_of_pass(k)) {
            if (t.off >= M) continue;
            p.consts[p.nterms] = t.c;
            p.off[p.nterms++] = t.off;
        }
        if (p.nterms == 0) {        // nothing reaches back into the quotient: the factor is 1 on this range
            if (src != dst && (rc = copy_d2d(dst, src, M * 8)) != IOPX_OK) return rc;
            src = dst;
            continue;
        }
        p.src = src; p.dst = dst; p.M = M;
        { ProfScope ps_("k64_polydiv_pass", 2 * M * 8); hipLaunchKernelGGL(k64_polydiv_pass, dim3(ops64_grid(M)), dim3(256), 0, stream(), p); }
        IOPX_HIP(hipGetLastError());
        src = dst;
    }
    return IOPX_OK;
}

static int lincomb64(const void *const *d_oracles, size_t num, const uint64_t *coeffs, const uint64_t *constant, size_t n, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_oracles || !coeffs || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (num == 0 || num > LINCOMB64_MAX) return fail(IOPX_ERR_INVALID_ARGUMENT, "Random Linear Combination Oracle: Expected same number of evaluations as in registration.");
    LincombParams64 p;
    memset(&p, 0, sizeof(p));
    bool pairs = aligned16(d_out);
    for (size_t i = 0; i < num; ++i) {
        if (!d_oracles[i]) return fail(IOPX_ERR_INVALID_ARGUMENT, "null oracle");
        p.o[i] = (const uint64_t *)d_oracles[i];
        p.c[i] = coeffs[i];
        pairs = pairs && aligned16(d_oracles[i]);
    }
    p.constant = constant ? constant[0] : 0;
    p.out = d_out; p.num = (int)num; p.n = n;
    if (n == 0) return IOPX_OK;
    ProfScope ps_("k64_lincomb", (num + 1) * n * 8);
    if (pairs) hipLaunchKernelGGL(k64_lincomb<2>, dim3(ops64_grid((n + 1) / 2)), dim3(256), 0, stream(), p);
    else hipLaunchKernelGGL(k64_lincomb<1>, dim3(ops64_grid(n)), dim3(256), 0, stream(), p);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

} // namespace iopx

using namespace iopx;

extern "C" {

int iopx_gf64_add_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (count == 0) return IOPX_OK;
    if (!d_a || !d_b || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    ProfScope ps_("k64_add", 3 * count * 8);
    if (aligned16(d_a) && aligned16(d_b) && aligned16(d_out)) hipLaunchKernelGGL(k64_add<2>, dim3(ops64_grid((count + 1) / 2)), dim3(256), 0, stream(), d_out, d_a, d_b, count);
    else hipLaunchKernelGGL(k64_add<1>, dim3(ops64_grid(count)), dim3(256), 0, stream(), d_out, d_a, d_b, count);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

// d_out[l] = init * base^l for l < count
int iopx_gf64_pow_table_dev(uint64_t *d_out, size_t count, const uint64_t *base, const uint64_t *init)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_out || !base || !init) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (count == 0) return IOPX_OK;
    PowParams64 p;
    memset(&p, 0, sizeof(p));
    p.nbits = (int)ceil_log2(count);
    if (p.nbits > POW64_MAX_BITS) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension too large");
    hgf64 x(base[0]);
    for (int k = 0; k < p.nbits; ++k) { p.sq[k] = x.v; x = x.squared(); }
    p.init = init[0];
    { ProfScope ps_("k64_pow_table", count * 8); hipLaunchKernelGGL(k64_pow_table, dim3(ops64_grid(count)), dim3(256), 0, stream(), d_out, count, p); }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

int iopx_lincomb_gf64_dev(const void *const *d_oracles, size_t num_oracles, const uint64_t *coefficients, size_t n, uint64_t *d_out)
{
    return lincomb64(d_oracles, num_oracles, coefficients, nullptr, n, d_out);
}

int iopx_lincomb_affine_gf64_dev(const void *const *d_oracles, size_t num_oracles, const uint64_t *coefficients, const uint64_t *constant, size_t n,
                                 uint64_t *d_out)
{
    if (!constant) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    return lincomb64(d_oracles, num_oracles, coefficients, constant, n, d_out);
}

int iopx_spmv_gf64_dev(const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_coeff, size_t rows, const uint64_t *d_vec,
                       const uint64_t *scale, int accumulate, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (rows == 0) return IOPX_OK;
    if (!d_row_ptr || !d_col || !d_coeff || !d_vec || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    SpmvParams64 p;
    p.row_ptr = d_row_ptr; p.col = d_col; p.coeff = d_coeff; p.vec = d_vec; p.out = d_out; p.rows = rows; p.accumulate = accumulate;
    p.has_scale = scale ? 1 : 0; p.scale = scale ? scale[0] : 0;
    // the entries are counted on the device only: the rows' output is what the host can declare
    { ProfScope ps_("k64_spmv", (size_t)(accumulate ? 2 : 1) * rows * 8); hipLaunchKernelGGL(k64_spmv, dim3(ops64_grid(rows)), dim3(256), 0, stream(), p); }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

int iopx_lincheck_gf64_dev(const uint64_t *d_fz, const void *const *d_Mz, size_t num_matrices, const uint64_t *r_Mz,
                           const uint64_t *d_p_alpha_prime, const uint64_t *d_p_alpha_ABC, size_t n, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_fz || !d_Mz || !r_Mz || !d_p_alpha_prime || !d_p_alpha_ABC || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (num_matrices == 0 || num_matrices > LINCHECK64_MAX_MATRICES)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "multi_lincheck uses more constituent oracles than what was provided.");
    LincheckParams64 p;
    memset(&p, 0, sizeof(p));
    p.fz = d_fz; p.p1 = d_p_alpha_prime; p.p2 = d_p_alpha_ABC; p.out = d_out;
    bool pairs = aligned16(d_fz) && aligned16(d_p_alpha_prime) && aligned16(d_p_alpha_ABC) && aligned16(d_out);
    for (size_t m = 0; m < num_matrices; ++m) {
        if (!d_Mz[m]) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
        p.mz[m] = (const uint64_t *)d_Mz[m];
        p.r[m] = r_Mz[m];
        pairs = pairs && aligned16(d_Mz[m]);
    }
    p.num_matrices = (int)num_matrices; p.n = n;
    if (n == 0) return IOPX_OK;
    ProfScope ps_("k64_lincheck", (num_matrices + 4) * n * 8);
    if (pairs) hipLaunchKernelGGL(k64_lincheck<2>, dim3(ops64_grid((n + 1) / 2)), dim3(256), 0, stream(), p);
    else hipLaunchKernelGGL(k64_lincheck<1>, dim3(ops64_grid(n)), dim3(256), 0, stream(), p);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

int iopx_rowcheck_gf64_dev(const uint64_t *d_Az, const uint64_t *d_Bz, const uint64_t *d_Cz, const uint64_t *basis, size_t m,
                           const uint64_t *shift, size_t constraint_dim, const uint64_t *constraint_shift, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_Az || !d_Bz || !d_Cz || !d_out || (m > 0 && !basis) || !shift || !constraint_shift) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (constraint_dim > m || m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "the constraint domain must be a sub-domain of the codeword domain");
    const size_t h = constraint_dim;
    TmpBuf dz;
    if ((rc = vanishing_inverse_table64(basis, m, shift, h, constraint_shift, dz)) != IOPX_OK) return rc;
    const size_t n = (size_t)1 << m;
    ProfScope ps_("k64_rowcheck", 4 * n * 8);
    if (aligned16(d_Az) && aligned16(d_Bz) && aligned16(d_Cz) && aligned16(d_out))
        hipLaunchKernelGGL(k64_rowcheck<2>, dim3(ops64_grid((n + 1) / 2)), dim3(256), 0, stream(), d_out, d_Az, d_Bz, d_Cz, (const uint64_t *)dz.u64(), (int)h, n);
    else
        hipLaunchKernelGGL(k64_rowcheck<1>, dim3(ops64_grid(n)), dim3(256), 0, stream(), d_out, d_Az, d_Bz, d_Cz, (const uint64_t *)dz.u64(), (int)h, n);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

int iopx_fz_gf64_dev(const uint64_t *d_fw, const uint64_t *d_f1v, const uint64_t *basis, size_t m, const uint64_t *shift,
                     const uint64_t *input_basis, size_t input_dim, const uint64_t *input_shift, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_fw || !d_f1v || !d_out || (m > 0 && !basis) || !shift || (input_dim > 0 && !input_basis) || !input_shift)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (input_dim > m || m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "Codeword domain must be bigger than the input variable domain.");
    // the subset-sum table of Z_I over the codeword domain: a function of the two domains only, kept on the device
    TmpBuf dt;
    rc = cached_domain_table(table_key64(basis, m, shift, input_basis, input_dim, input_shift, 0x3634667a), [&](std::vector<uint64_t> &tab) -> int {     // "64fz"
        const std::vector<hgf64> ib = host_elems64(input_basis, input_dim);
        const SubspacePoly64 lin(ib.data(), input_dim);                                    // Z_I's linear part
        tab.push_back((lin.eval(hgf64(shift[0])) + lin.eval(hgf64(input_shift[0]))).v);     // Z_I(shift) = lin(shift) + lin(shift_I)
        for (size_t k = 0; k < m; ++k) tab.push_back(lin.eval(hgf64(basis[k])).v);
        return IOPX_OK;
    }, dt);
    if (rc != IOPX_OK) return rc;
    const size_t n = (size_t)1 << m;
    ProfScope ps_("k64_fz", 3 * n * 8);
    if (aligned16(d_fw) && aligned16(d_f1v) && aligned16(d_out))
        hipLaunchKernelGGL(k64_fz<2>, dim3(ops64_grid((n + 1) / 2)), dim3(256), 0, stream(), d_out, d_fw, d_f1v, (const uint64_t *)dt.u64(), (int)m, n);
    else
        hipLaunchKernelGGL(k64_fz<1>, dim3(ops64_grid(n)), dim3(256), 0, stream(), d_out, d_fw, d_f1v, (const uint64_t *)dt.u64(), (int)m, n);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

int iopx_sumcheck_g_gf64_dev(const uint64_t *d_f, const uint64_t *d_h, const uint64_t *basis, size_t m, const uint64_t *shift,
                             const uint64_t *summation_basis, size_t summation_dim, const uint64_t *summation_shift,
                             const uint64_t *claimed_sum, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_f || !d_h || !d_out || (m > 0 && !basis) || !shift || (summation_dim > 0 && !summation_basis) || !summation_shift || !claimed_sum)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (m > 40 || summation_dim > 63) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension too large");
    const std::vector<hgf64> sb = host_elems64(summation_basis, summation_dim);
    const SubspacePoly64 lin(sb.data(), summation_dim);                                    // Z_H's linear part
    if (lin.coeff[0].is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "the summation domain's basis is linearly dependent");
    const hgf64 c = lin.coeff[0].inverse() * hgf64(claimed_sum[0]);                         // eps^-1 mu (sumcheck.tcc:52-54)
    // the subset-sum tables of x, x^|H| and Z_H(x) over the codeword domain: functions of the two domains only, kept on the device (one block)
    const size_t table_words = m + 1;
    TmpBuf dtabs;
    rc = cached_domain_table(table_key64(basis, m, shift, summation_basis, summation_dim, summation_shift, 0x363473756d), [&](std::vector<uint64_t> &words) -> int {   // "64sum"
        words.assign(3 * table_words, 0);
        for (size_t k = 0; k <= m; ++k) {
            const hgf64 v(k == 0 ? shift[0] : basis[k - 1]);
            hgf64 vh = v;
            for (size_t i = 0; i < summation_dim; ++i) vh = vh.squared();                  // v^|H|
            hgf64 vz = lin.eval(v);
            if (k == 0) vz += lin.eval(hgf64(summation_shift[0]));                         // Z_H(shift) = lin(shift) + lin(shift_H)
            words[k] = v.v; words[table_words + k] = vh.v; words[2 * table_words + k] = vz.v;
        }
        return IOPX_OK;
    }, dtabs);
    if (rc != IOPX_OK) return rc;
    SumcheckParams64 p;
    p.f = d_f; p.h = d_h; p.out = d_out;
    p.xtab = dtabs.u64(); p.htab = dtabs.u64() + table_words; p.ztab = dtabs.u64() + 2 * table_words;
    p.c = c.v; p.m = (int)m; p.n = (size_t)1 << m;
    const bool pairs = aligned16(d_f) && aligned16(d_h) && aligned16(d_out);
    const dim3 grid(ops64_grid(pairs ? (p.n + 1) / 2 : p.n));
    if (c.is_zero()) {
        ProfScope ps_("k64_sumcheck_g_zero_sum", 3 * p.n * 8);
        if (pairs) hipLaunchKernelGGL((k64_sumcheck_g<2, false>), grid, dim3(256), 0, stream(), p);
        else hipLaunchKernelGGL((k64_sumcheck_g<1, false>), grid, dim3(256), 0, stream(), p);
    } else {
        ProfScope ps_("k64_sumcheck_g", 3 * p.n * 8);
        if (pairs) hipLaunchKernelGGL((k64_sumcheck_g<2, true>), grid, dim3(256), 0, stream(), p);
        else hipLaunchKernelGGL((k64_sumcheck_g<1, true>), grid, dim3(256), 0, stream(), p);
    }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

int iopx_poly_div_vanishing_gf64_dev(const uint64_t *d_poly, size_t n_coeffs, const uint64_t *basis, size_t dim, const uint64_t *shift,
                                     uint64_t *d_quotient)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_poly || (dim > 0 && !basis) || !shift || !d_quotient) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (dim > 62) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension too large");
    const size_t N = (size_t)1 << dim;
    if (n_coeffs <= N) return IOPX_OK;                       // empty quotient (linearized_polynomial.tcc:247-255)
    const size_t M = n_coeffs - N;
    // Z = sum_{i <= dim} lin[i] X^(2^i) + lin(shift) (vanishing_polynomial.tcc:373-395)
    const std::vector<hgf64> b = host_elems64(basis, dim);
    const SubspacePoly64 lin(b.data(), dim);
    if (!(lin.coeff[dim] == hgf64::one())) return fail(IOPX_ERR_LOGIC, "vanishing polynomial is not monic");
    const hgf64 c_const = lin.eval(hgf64(shift[0]));
    std::vector<hgf64> cur;                                  // c_i^(2^k), squared once per pass
    std::vector<size_t> base_off;
    for (size_t i = 0; i < dim; ++i) if (!lin.coeff[i].is_zero()) { cur.push_back(lin.coeff[i]); base_off.push_back(N - ((size_t)1 << i)); }
    if (!c_const.is_zero()) { cur.push_back(c_const); base_off.push_back(N); }
    if (cur.size() > PDIV64_MAX_TERMS) return fail(IOPX_ERR_INVALID_ARGUMENT, "too many terms");
    size_t min_off = 0;
    for (size_t o : base_off) if (min_off == 0 || o < min_off) min_off = o;
    int done = 0;
    auto terms_of_pass = [&](int k) {
        while (done < k) { for (hgf64 &c : cur) c = c.squared(); ++done; }
        std::vector<Term64> t;
        for (size_t i = 0; i < cur.size(); ++i) {
            Term64 x;
            x.off = base_off[i] << k;
            x.c = cur[i].v;
            t.push_back(x);
        }
        return t;
    };
    return run_division64(d_poly + N, M, min_off, d_quotient, terms_of_pass);
}

// d_out[j] = d_in[j] / Z_S(x_j) over span(basis[0..m)) + shift, S = span(basis[0..sub_dim)) + sub_shift (d_out may be d_in).  The profile reports the
// one-element form (a vector that is not 16-byte aligned) as k64_div_by_vanishing_w64.
int iopx_div_by_vanishing_gf64_dev(const uint64_t *d_in, const uint64_t *basis, size_t m, const uint64_t *shift, size_t sub_dim, const uint64_t *sub_shift,
                                   uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_in || !d_out || (m > 0 && !basis) || !shift || !sub_shift) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (sub_dim > m || m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "the vanishing set must be spanned by a prefix of the domain's basis");
    TmpBuf dz;
    if ((rc = vanishing_inverse_table64(basis, m, shift, sub_dim, sub_shift, dz, 0x3634646976 /* "64div" */, "the domain intersects the vanishing set")) != IOPX_OK) return rc;
    const size_t n = (size_t)1 << m;
    if (aligned16(d_in) && aligned16(d_out)) {
        ProfScope ps_("k64_div_by_vanishing", 2 * n * 8);
        hipLaunchKernelGGL(k64_div_by_vanishing<2>, dim3(ops64_grid_capped((n + 1) / 2)), dim3(256), 0, stream(), d_out, d_in, (const uint64_t *)dz.u64(), (int)sub_dim, n);
    } else {
        ProfScope ps_("k64_div_by_vanishing_w64", 2 * n * 8);
        hipLaunchKernelGGL(k64_div_by_vanishing<1>, dim3(ops64_grid_capped(n)), dim3(256), 0, stream(), d_out, d_in, (const uint64_t *)dz.u64(), (int)sub_dim, n);
    }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

// Z_S(x) and Z_S's linear coefficient (its formal derivative, vanishing_polynomial.tcc:55-74) for S = span(basis) + shift: host only
int iopx_gf64_vanishing_host(const uint64_t *basis, size_t dim, const uint64_t *shift, const uint64_t *x, uint64_t *value_out, uint64_t *linear_coefficient_out)
{
    if ((dim > 0 && !basis) || !shift || !x) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (dim > 63) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension too large");
    const std::vector<hgf64> b = host_elems64(basis, dim);
    const SubspacePoly64 lin(b.data(), dim);
    if (value_out) value_out[0] = (lin.eval(hgf64(x[0])) + lin.eval(hgf64(shift[0]))).v;
    if (linear_coefficient_out) linear_coefficient_out[0] = lin.coeff[0].v;
    return IOPX_OK;
}

} // extern "C"
