// The protocol-layer steps of the encoded Aurora prover over a binary field, written once: the twins of encoded_ops.hip / virtual_oracles.hip
// for GF(2^64), GF(2^128) and GF(2^256).  gf64_ops.hip, gf128_ops.hip and gf256_ops.hip include this text and instantiate it for their element
// trait (gf64_elem.h, gf128_elem.h, gf256_elem.h; gfx_additive.h lists what a trait gives, and this text reads OPS_TAG besides: the tag of its
// cached domain tables).
//
//   x_add_dev, x_pow_table_dev                     the vector add, the powers of alpha (basic_lincheck_aux.tcc:37-45)
//   x_lincomb_dev                                  random_linear_combination_oracle::evaluated_contents (random_linear_combination.tcc:27-57),
//                                                  single_matrix_denominator::evaluated_contents (holographic_lincheck_aux.tcc:117-143)
//   x_spmv_dev                                     create_Az_Bz_Cz_from_variable_assignment (r1cs.tcc:236-268), p_alpha_ABC (basic_lincheck_aux.tcc:64-88)
//   x_lincheck_dev                                 multi_lincheck_virtual_oracle::evaluated_contents (basic_lincheck_aux.tcc:102-144)
//   x_rowcheck_dev                                 rowcheck_ABC_virtual_oracle::evaluated_contents (rowcheck.tcc:16-88)
//   x_fz_dev                                       fz_virtual_oracle::evaluated_contents (r1cs_rs_iop.tcc:181-222)
//   x_sumcheck_g_dev                               sumcheck_g_oracle::evaluated_contents (sumcheck.tcc:58-119)
//   x_poly_div_vanishing_dev                       polynomial_over_vanishing_polynomial(...).first (vanishing_polynomial.tcc:314-371)
//   x_div_by_vanishing_dev, x_vanishing_host       the head route's pointwise division by Z_S and the host's Z_S(x) (include/libiop_amd_head.h)
//   x_div_dev, x_domain_offsets_dev, x_vanishing_evals_dev, x_rational_combine_dev, x_rational_sumcheck_constraint_dev
//                                                  the holographic prover's steps, the twins of fractal_ops.hip (include/libiop_amd_fractal.h)
//
// Every kernel reads each input once and writes the output once, in a grid-stride loop.  An element travels as F::mem through F::load<A16> /
// F::store<A16>: the A16 instantiation (16-byte accesses) runs when every device pointer that it reads or writes 16 bytes at a time is 16-byte
// aligned, the other one (64-bit words, "_w64" in the profile) otherwise.  A lane takes one element; in the 16-byte form over a one-word
// element it takes the two consecutive elements of one access (ops_lane) where the position of an element does not enter the addressing
// beyond "j and j + 1": everywhere but the powers of a base, the CSR gather and the division passes (odd offsets), which have one form over
// such an element and the plain name.  Constants of a launch (coefficients, the squares of a base, the terms of a division pass) travel in
// the kernel's argument block: no upload.  The domain-shaped values Z_I(x_j), Z_H(x_j), x_j, x_j^|H| are subset sums of an (m + 1)-entry
// table over the bits of j (linearized_polynomial.tcc:83-108); position j + 1 of a pair differs from position j by the table's entry for
// bit 0.  No LDS but the product tree of the batch division (kx_div).  The grid is capped by the option IOPX_GFX_OPS_MAX_BLOCKS (default 16384, looked up per launch; a test helper: a small cap
// sends every grid-stride loop round again at a few thousand elements).
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>
#include <vector>
#include "runtime.h"
#include "subspace_poly.h"

namespace iopx {

static int ops_grid_x(size_t work)
{
    const size_t cap = (size_t)opt_range("IOPX_GFX_OPS_MAX_BLOCKS", 16384, 1, 16384);
    size_t g = (work + 255) / 256;
    if (g > cap) g = cap;
    return (int)(g ? g : 1);
}

static bool ops_al16(const void *p) { return (((uintptr_t)p) & 15) == 0; }
// a cached table is read one element at a time: a one-word element asks no alignment of it
template<class F> static bool ops_table_al16(const void *p) { return F::W == 1 || ops_al16(p); }

// elements per lane in the 16-byte form: two one-word elements fill one access.  The kernels written over a lane's elements (LaneX below)
// take ops_lane<F, A16>: one for every wider element and in the 64-bit-word form.
template<class F, bool A16> constexpr int ops_lane = A16 && F::W == 1 ? 2 : 1;

// Launch K over `work` elements: K<F, true> (`lane` elements per lane: ops_lane<F, true> for a kernel written over a lane's elements, 1 for
// the others) when `a16`, K<F, false> otherwise, under the matching profile name: the field's stem + the kernel's name (+ "_w64"), built once
// per launch site and field.  Where the two would be the same code (a one-word element, one element per lane) there is one instantiation
// and one name, without "_w64".
#define IOPX_OPS_LAUNCH(a16, name, bytes, K, lane, work, ...) IOPX_OPS_LAUNCH_ON(a16, name, bytes, K, lane, work, ops_grid_x, 0, __VA_ARGS__)
// ... with the grid as GRID(slots of `lane` elements) and `lds` bytes of dynamic LDS
#define IOPX_OPS_LAUNCH_ON(a16, name, bytes, K, lane, work, GRID, lds, ...)                                            \
    do {                                                                                                               \
        constexpr size_t lane_ = (lane);                                                                               \
        constexpr bool forms_ = F::W > 1 || lane_ > 1;                                                                 \
        const bool a16_ = forms_ && (a16);                                                                             \
        static const std::string names_[2] = { std::string(F::stem()) + name, std::string(F::stem()) + name + "_w64" }; \
        ProfScope ps_(names_[forms_ && !a16_ ? 1 : 0].c_str(), bytes);                                                 \
        const dim3 grid_(GRID(a16_ ? ((work) + lane_ - 1) / lane_ : (work)));                                          \
        if constexpr (forms_) {                                                                                        \
            if (a16_) hipLaunchKernelGGL((K<F, true>), grid_, dim3(256), lds, stream(), __VA_ARGS__);                  \
            else hipLaunchKernelGGL((K<F, false>), grid_, dim3(256), lds, stream(), __VA_ARGS__);                      \
        } else {                                                                                                       \
            hipLaunchKernelGGL((K<F, false>), grid_, dim3(256), lds, stream(), __VA_ARGS__);                           \
        }                                                                                                              \
    } while (0)

// a grid-stride loop of V elements per lane: j is a multiple of V
#define OPSX_LOOP_V(V, j, n) \
    for (size_t j = (size_t)(V) * ((size_t)blockIdx.x * blockDim.x + threadIdx.x); j < (n); j += (size_t)(V) * gridDim.x * blockDim.x)
#define OPSX_LOOP(j, n) OPSX_LOOP_V(1, j, n)

// t[0] + sum_{bit k of j} t[1 + k], j < 2^m
template<class F, bool A16>
__device__ __forceinline__ typename F::mem subset_sum_x(const uint64_t *t, int m, size_t j)
{
    typename F::mem v = F::template load<A16>(t, 0);
    for (int k = 0; k < m; ++k) if ((j >> k) & 1) v = F::add(v, F::template load<A16>(t, 1 + k));
    return v;
}

// The elements [j, j + V) of one lane as a value (val) and the field's operations on it: what a kernel over a lane's elements is written in.
// An operand of the arithmetic may be named ahead of it (fetch) and read where it is used (get), for the sake of the pair form below.
//
// One element per lane: val is the element, every operation is the field's own, and an operand is fetched where it is used.  The kernels
// then are the text they were before the pair form, and the code of the wider fields is the code it was.
template<class F, bool A16, int V = ops_lane<F, A16>>
struct LaneX : F {
    static_assert(V == 1, "one element per lane, or the pair form below");
    typedef typename F::mem mem;
    typedef mem val;
    typedef const uint64_t *operand;
    static __device__ __forceinline__ val load(const uint64_t *p, size_t j, size_t) { return F::template load<A16>(p, j); }
    static __device__ __forceinline__ void store(uint64_t *p, size_t j, size_t, const val &x) { F::template store<A16>(p, j, x); }
    static __device__ __forceinline__ operand fetch(const uint64_t *p, size_t, size_t) { return p; }
    static __device__ __forceinline__ val get(operand p, size_t j, size_t) { return F::template load<A16>(p, j); }
    static __device__ __forceinline__ const mem &splat(const mem &c) { return c; }
    // zinv[j >> s], the entry of the position's coset: named (coset) and read where it is used (entry), as an operand
    struct cosets { const uint64_t *zinv; size_t j; int s; };
    static __device__ __forceinline__ cosets coset(const uint64_t *zinv, size_t j, int s, size_t) { cosets z; z.zinv = zinv; z.j = j; z.s = s; return z; }
    static __device__ __forceinline__ val entry(const cosets &z) { return F::template load<A16>(z.zinv, z.j >> z.s); }
    static __device__ __forceinline__ val sums(const uint64_t *t, int m, size_t j) { return subset_sum_x<F, A16>(t, m, j); }
    // add, mul and inv are F's functions themselves (hence the base class), not wrappers of them: behind a wrapper's extra level of inlining
    // the compiler swapped the operands of a few commutative instructions in the products of the wider fields
    using F::add;
    using F::mul;
    using F::inv;
};

// Two one-word elements per lane, j even.  Position j + 1 is absent at the end of an odd n: it reads as zero and is not written.  A pair is
// fetched where it is named: its accesses sit in branches of their own (the absent position), which the compiler does not move, so fetched at
// their uses they would wait behind the arithmetic in front of them.
struct alignas(16) OpsPair { uint64_t a, b; };

template<class F, bool A16>
struct LaneX<F, A16, 2> {
    static constexpr int V = 2;
    typedef typename F::mem mem;
    struct val { mem e[V]; };
    typedef val operand;

    static __device__ __forceinline__ val load(const uint64_t *p, size_t j, size_t n)
    {
        val r;
        if (j + 1 < n) { const OpsPair t = *reinterpret_cast<const OpsPair *>(p + j); r.e[0] = t.a; r.e[1] = t.b; }
        else { r.e[0] = p[j]; r.e[1] = 0; }
        return r;
    }
    static __device__ __forceinline__ void store(uint64_t *p, size_t j, size_t n, const val &x)
    {
        if (j + 1 < n) { OpsPair t; t.a = x.e[0]; t.b = x.e[1]; *reinterpret_cast<OpsPair *>(p + j) = t; }
        else p[j] = x.e[0];
    }
    static __device__ __forceinline__ operand fetch(const uint64_t *p, size_t j, size_t n) { return load(p, j, n); }
    static __device__ __forceinline__ const val &get(const operand &x, size_t, size_t) { return x; }
    // one value of the launch in both positions
    static __device__ __forceinline__ val splat(const mem &c) { val r; r.e[0] = c; r.e[1] = c; return r; }
    // zinv[(j + e) >> s], the entry of each position's coset, fetched where it is named.  The absent position has none, and a product with
    // the entries leaves that position as it is (a branch per element: the two products one after the other take 54 registers in rowcheck,
    // side by side 69)
    struct cosets { mem e[V]; size_t j, n; };
    static __device__ __forceinline__ cosets coset(const uint64_t *zinv, size_t j, int s, size_t n)
    {
        cosets z;
        z.j = j; z.n = n;
#pragma unroll
        for (int e = 0; e < V; ++e) z.e[e] = j + e < n ? F::template load<A16>(zinv, (j + e) >> s) : F::zero();
        return z;
    }
    static __device__ __forceinline__ const cosets &entry(const cosets &z) { return z; }
    static __device__ __forceinline__ val mul(const val &a, const cosets &z)
    {
        val r = a;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if (z.j + e < z.n) r.e[e] = F::mul(a.e[e], z.e[e]);
        }
        return r;
    }
    // the subset sums at positions j and j + 1: the second is the first plus the entry for bit 0, which the table of a domain of one element
    // does not have (there position j + 1 is absent)
    static __device__ __forceinline__ val sums(const uint64_t *t, int m, size_t j)
    {
        val r;
        r.e[0] = subset_sum_x<F, A16>(t, m, j);
        r.e[1] = m > 0 ? F::add(r.e[0], F::template load<A16>(t, 1)) : F::zero();
        return r;
    }
    static __device__ __forceinline__ val add(const val &a, const val &b) { val r; r.e[0] = F::add(a.e[0], b.e[0]); r.e[1] = F::add(a.e[1], b.e[1]); return r; }
    static __device__ __forceinline__ val mul(const val &a, const val &b) { val r; r.e[0] = F::mul(a.e[0], b.e[0]); r.e[1] = F::mul(a.e[1], b.e[1]); return r; }
    static __device__ __forceinline__ val inv(const val &a) { val r; r.e[0] = F::inv(a.e[0]); r.e[1] = F::inv(a.e[1]); return r; }
};

// ---- elementwise -----------------------------------------------------------------------------------------------------------
template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_add(uint64_t *out, const uint64_t *a, const uint64_t *b, size_t n)
{
    typedef LaneX<F, A16> L;
    OPSX_LOOP_V((ops_lane<F, A16>), j, n) L::store(out, j, n, L::add(L::load(a, j, n), L::load(b, j, n)));
}

// ---- the powers of a base -------------------------------------------------------------------------------------------------
// out[l] = init * base^l: the product of sq[k] = base^(2^k) over the set bits of l
#define POWX_MAX_BITS 40
template<class F>
struct PowParamsX {
    typename F::mem sq[POWX_MAX_BITS];
    typename F::mem init;
    int nbits;
};

template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_pow_table(uint64_t *out, size_t count, PowParamsX<F> p)
{
    OPSX_LOOP(l, count) {
        typename F::reg acc = F::unpack(p.init);
        for (int k = 0; k < p.nbits; ++k) {
            if ((l >> k) & 1) acc = F::rmul(acc, F::unpack(p.sq[k]));
        }
        F::template store<A16>(out, l, F::pack(acc));
    }
}

// ---- random linear combination ---------------------------------------------------------------------------------------------
#define LINCOMBX_MAX 16
template<class F>
struct LincombParamsX {
    const uint64_t *o[LINCOMBX_MAX];
    typename F::mem c[LINCOMBX_MAX];
    typename F::mem constant;   // zero when there is none
    uint64_t *out;
    int num;
    size_t n;
};

template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_lincomb(LincombParamsX<F> p)
{
    typedef LaneX<F, A16> L;
    OPSX_LOOP_V((ops_lane<F, A16>), j, p.n) {
        typename L::val acc = L::splat(p.constant);
        for (int i = 0; i < p.num; ++i) acc = L::add(acc, L::mul(L::load(p.o[i], j, p.n), L::splat(p.c[i])));
        L::store(p.out, j, p.n, acc);
    }
}

// ---- CSR sparse matrix x vector: one lane per row ----------------------------------------------------------------------------
template<class F>
struct SpmvParamsX {
    const uint64_t *row_ptr;    // rows + 1 offsets
    const uint32_t *col;
    const uint64_t *coeff, *vec;
    uint64_t *out;
    typename F::mem scale;
    size_t rows;
    int has_scale, accumulate;
};

template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_spmv(SpmvParamsX<F> p)
{
    OPSX_LOOP(r, p.rows) {
        typename F::mem acc = F::zero();
        const uint64_t e = p.row_ptr[r + 1];
        for (uint64_t t = p.row_ptr[r]; t < e; ++t) acc = F::add(acc, F::mul(F::template load<A16>(p.vec, p.col[t]), F::template load<A16>(p.coeff, t)));
        if (p.has_scale) acc = F::mul(acc, p.scale);
        if (p.accumulate) acc = F::add(acc, F::template load<A16>(p.out, r));
        F::template store<A16>(p.out, r, acc);
    }
}

// ---- one factor (1 + u^(2^k)) of the power-series inverse (encoded_ops.hip) --------------------------------------------------
#define PDIVX_MAX_TERMS 66
template<class F>
struct PolyDivParamsX {
    const uint64_t *src;
    uint64_t *dst;
    typename F::mem consts[PDIVX_MAX_TERMS];
    size_t off[PDIVX_MAX_TERMS];
    size_t M;
    int nterms;
};

template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_polydiv_pass(PolyDivParamsX<F> p)
{
    OPSX_LOOP(j, p.M) {
        typename F::mem acc = F::template load<A16>(p.src, j);
        for (int t = 0; t < p.nterms; ++t) {
            const size_t s = j + p.off[t];
            if (s < p.M) acc = F::add(acc, F::mul(F::template load<A16>(p.src, s), p.consts[t]));
        }
        F::template store<A16>(p.dst, j, acc);
    }
}

// ---- virtual oracles -----------------------------------------------------------------------------------------------------
// result[x] = (Az(x) Bz(x) - Cz(x)) / Z_H(x); cosets of H are the blocks position >> h of the codeword domain (virtual_oracles.hip)
template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_rowcheck(uint64_t *out, const uint64_t *az, const uint64_t *bz, const uint64_t *cz, const uint64_t *zinv, int h,
                                                   size_t n)
{
    typedef LaneX<F, A16> L;
    OPSX_LOOP_V((ops_lane<F, A16>), j, n) {
        const typename L::operand a = L::fetch(az, j, n), b = L::fetch(bz, j, n), c = L::fetch(cz, j, n);
        const typename L::cosets z = L::coset(zinv, j, h, n);
        const typename L::val ab = L::mul(L::get(a, j, n), L::get(b, j, n));
        // characteristic 2: a b - c = a b + c
        L::store(out, j, n, L::mul(L::add(ab, L::get(c, j, n)), L::entry(z)));
    }
}

// out[x] = in[x] / Z_S(x): Z_S is constant on the cosets of S, the blocks position >> s of the domain; one product per element, out may be in
template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_div_by_vanishing(uint64_t *out, const uint64_t *in, const uint64_t *zinv, int s, size_t n)
{
    typedef LaneX<F, A16> L;
    OPSX_LOOP_V((ops_lane<F, A16>), j, n) L::store(out, j, n, L::mul(L::load(in, j, n), L::entry(L::coset(zinv, j, s, n))));
}

// result[x] = fw(x) Z_I(x) + f_1v(x)
template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_fz(uint64_t *out, const uint64_t *fw, const uint64_t *f1v, const uint64_t *tab, int m, size_t n)
{
    typedef LaneX<F, A16> L;
    OPSX_LOOP_V((ops_lane<F, A16>), j, n) {
        const typename L::operand w = L::fetch(fw, j, n), f = L::fetch(f1v, j, n);
        const typename L::val z = L::sums(tab, m, j);
        L::store(out, j, n, L::add(L::mul(L::get(w, j, n), z), L::get(f, j, n)));
    }
}

// p'(x) = f(x) - eps^-1 mu x^(|H| - 1) - Z_H(x) h(x), x^(|H| - 1) = x^|H| / x with 1 / 0 = 0 (sumcheck_aux.tcc:3-32, utils.tcc:79-97).
// NONZERO = false is the arm every shipped protocol takes (claimed sum 0: no middle term, no inversion).  The other arm inverts each
// x_j directly (F::inv maps 0 to 0): no staging in LDS and no per-lane batch.
template<class F>
struct SumcheckParamsX {
    const uint64_t *f, *h;
    uint64_t *out;
    const uint64_t *xtab, *htab, *ztab;     // (m + 1)-entry subset-sum tables of x, x^|H|, Z_H(x)
    typename F::mem c;                      // eps^-1 mu
    int m;
    size_t n;
};

template<class F, bool A16, bool NONZERO>
__device__ __forceinline__ void sumcheck_g_body(const SumcheckParamsX<F> &p)
{
    typedef LaneX<F, A16> L;
    OPSX_LOOP_V((ops_lane<F, A16>), j, p.n) {
        const typename L::operand h = L::fetch(p.h, j, p.n);
        typename L::val f = L::load(p.f, j, p.n);
        f = L::add(f, L::mul(L::sums(p.ztab, p.m, j), L::get(h, j, p.n)));
        if constexpr (NONZERO) {
            const typename L::val xinv_c = L::mul(L::inv(L::sums(p.xtab, p.m, j)), L::splat(p.c));
            f = L::add(f, L::mul(L::sums(p.htab, p.m, j), xinv_c));
        }
        L::store(p.out, j, p.n, f);
    }
}
template<class F, bool A16> __global__ void __launch_bounds__(256) kx_sumcheck_g_zero_sum(SumcheckParamsX<F> p) { sumcheck_g_body<F, A16, false>(p); }
template<class F, bool A16> __global__ void __launch_bounds__(256) kx_sumcheck_g(SumcheckParamsX<F> p) { sumcheck_g_body<F, A16, true>(p); }

// result[x] = (sum_m r_m Mz_m(x)) p_alpha^1(x) - fz(x) p_alpha^2(x)
#define LINCHECKX_MAX_MATRICES 8
template<class F>
struct LincheckParamsX {
    const uint64_t *fz, *p1, *p2;
    const uint64_t *mz[LINCHECKX_MAX_MATRICES];
    typename F::mem r[LINCHECKX_MAX_MATRICES];
    uint64_t *out;
    int num_matrices;
    size_t n;
};

template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_lincheck(LincheckParamsX<F> p)
{
    typedef LaneX<F, A16> L;
    OPSX_LOOP_V((ops_lane<F, A16>), j, p.n) {
        typename L::val comb = L::splat(F::zero());
        for (int m = 0; m < p.num_matrices; ++m) comb = L::add(comb, L::mul(L::load(p.mz[m], j, p.n), L::splat(p.r[m])));
        comb = L::mul(comb, L::load(p.p1, j, p.n));
        comb = L::add(comb, L::mul(L::load(p.fz, j, p.n), L::load(p.p2, j, p.n)));
        L::store(p.out, j, p.n, comb);
    }
}

// ---- the holographic (Fractal) prover's steps: the twins of fractal_ops.hip ------------------------------------------------------
template<class F>
__device__ __forceinline__ bool ops_is_zero(const typename F::mem &v)
{
    if constexpr (F::W == 1) return v == 0;
    else {
        uint64_t any = 0;
#pragma unroll
        for (int i = 0; i < F::W; ++i) any |= v.w[i];
        return any == 0;
    }
}

// the V elements of a lane's value, one by one (LaneX<F, A16, V>::val is the element itself at V = 1)
template<class F, bool A16, int V>
__device__ __forceinline__ void lane_split(const typename LaneX<F, A16, V>::val &x, typename F::mem (&e)[V])
{
    if constexpr (V == 1) e[0] = x;
    else {
#pragma unroll
        for (int i = 0; i < V; ++i) e[i] = x.e[i];
    }
}
template<class F, bool A16, int V>
__device__ __forceinline__ typename LaneX<F, A16, V>::val lane_join(const typename F::mem (&e)[V])
{
    if constexpr (V == 1) return e[0];
    else {
        typename LaneX<F, A16, V>::val x;
#pragma unroll
        for (int i = 0; i < V; ++i) x.e[i] = e[i];
        return x;
    }
}

// out[j] = num[j] / den[j] (num null: 1 / den[j]; a zero denominator yields zero, utils.tcc:79-97) by Montgomery's trick, as k_div_gf192: a logical
// lane walks the slots lane, lane + T, ... of the launch (a slot: the V consecutive elements of one access), parks its running products in the
// OUTPUT on the way up and consumes them on the way down; the 256 lanes of a workgroup combine their totals in an LDS tree (511 nodes), so a
// workgroup pays for ONE field inversion (lane 0's serial work).  A zero denominator, and the absent position at the end of an odd n, is stepped
// over as a one.  Written over logical lanes, so that any block size runs the same arithmetic.
template<class F>
struct DivParamsX {
    const uint64_t *num;        // nullable
    const uint64_t *den;
    uint64_t *out;              // distinct from num and den
    size_t n;
};

static constexpr unsigned DIVX_LANES = 256, DIVX_TREE_NODES = 2 * DIVX_LANES - 1, DIVX_SLOTS_PER_LANE = 16, DIVX_MAX_BLOCKS = 2048;
__device__ __forceinline__ unsigned divx_level_base(int l) { return 2 * DIVX_LANES - ((2 * DIVX_LANES) >> l); }

// a^-1 for a != 0 by the binary extended Euclidean algorithm on polynomials over GF(2), as gf_inv_euclid of fractal_ops.hip: g a = u and h a = v
// modulo the field's polynomial f = x^(64 W) + F::MODULUS_LOW, and the one of higher degree absorbs a shifted copy of the other until u = 1; at most
// 2 * 64 W shift-and-XOR steps on W + 1 words, for the ONE lane that inverts a workgroup's root.  Every index below is a constant once the loops are
// unrolled, so the four values stay in registers (no scratch memory: the register report of DESIGN.md §5.18).
template<int N>
__device__ __forceinline__ int poly_degree(const uint64_t (&x)[N])
{
    int d = -1;
#pragma unroll
    for (int i = 0; i < N; ++i) if (x[i]) d = 64 * i + 63 - __builtin_clzll(x[i]);
    return d;
}
template<int N>
__device__ __forceinline__ void poly_xor_shifted(uint64_t (&x)[N], const uint64_t (&y)[N], int j)
{
    const int bs = j & 63, ws = j >> 6;
    uint64_t t[N];
#pragma unroll
    for (int i = 0; i < N; ++i) t[i] = bs ? (y[i] << bs) | (i ? y[i - 1] >> (64 - bs) : 0) : y[i];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        if (ws == c) {
#pragma unroll
            for (int i = 0; i + c < N; ++i) x[i + c] ^= t[i];
        }
    }
}
template<class F>
__device__ inline typename F::mem ops_inv_euclid(const typename F::mem &a)
{
    constexpr int W = F::W, N = W + 1;
    uint64_t u[N], v[N], g[N], h[N];
    memcpy(u, &a, 8 * W);                   // F::mem is W words
    u[W] = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) { v[i] = 0; g[i] = 0; h[i] = 0; }
    v[0] = F::MODULUS_LOW; v[W] = 1; g[0] = 1;
    int du = poly_degree<N>(u), dv = 64 * W;
    while (du > 0) {
        int j = du - dv;
        if (j < 0) {
#pragma unroll
            for (int i = 0; i < N; ++i) { uint64_t t = u[i]; u[i] = v[i]; v[i] = t; t = g[i]; g[i] = h[i]; h[i] = t; }
            const int d = du; du = dv; dv = d;
            j = -j;
        }
        poly_xor_shifted<N>(u, v, j);
        poly_xor_shifted<N>(g, h, j);
        du = poly_degree<N>(u);
    }
    typename F::mem r;
    memcpy(&r, g, 8 * W);
    return r;
}

// EUCLID: the root is inverted by ops_inv_euclid, otherwise by the field's Fermat power (F::inv)
template<class F, bool A16, bool EUCLID>
__device__ __forceinline__ void div_body(const DivParamsX<F> &p)
{
    constexpr int V = ops_lane<F, A16>;
    typedef LaneX<F, A16> L;
    typedef typename F::mem mem;
    extern __shared__ __attribute__((aligned(16))) uint64_t iopx_smem[];
    mem *tree = reinterpret_cast<mem *>(iopx_smem);
    const size_t T = (size_t)gridDim.x * DIVX_LANES;
    const size_t slots = (p.n + V - 1) / V;
    const mem one = F::one();
    const unsigned tid = threadIdx.x, nt = blockDim.x;      // read once, as the other LDS kernels do
    for (unsigned lane = tid; lane < DIVX_LANES; lane += nt) {
        mem run = one;
        for (size_t s = (size_t)blockIdx.x * DIVX_LANES + lane; s < slots; s += T) {
            mem d[V];
            lane_split<F, A16, V>(L::load(p.den, V * s, p.n), d);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if (!ops_is_zero<F>(d[e])) run = F::mul(run, d[e]);
                d[e] = run;
            }
            L::store(p.out, V * s, p.n, lane_join<F, A16, V>(d));
        }
        tree[lane] = run;
    }
    __syncthreads();
    for (int l = 1; (DIVX_LANES >> l) >= 1; ++l) {
        const unsigned cnt = DIVX_LANES >> l, base = divx_level_base(l), below = divx_level_base(l - 1);
        for (unsigned i = tid; i < cnt; i += nt) tree[base + i] = F::mul(tree[below + 2 * i], tree[below + 2 * i + 1]);
        __syncthreads();
    }
    if (tid == 0) tree[DIVX_TREE_NODES - 1] = EUCLID ? ops_inv_euclid<F>(tree[DIVX_TREE_NODES - 1]) : F::inv(tree[DIVX_TREE_NODES - 1]);   // never zero: a product of non-zero elements
    __syncthreads();
    for (int l = 8; l >= 1; --l) {
        const unsigned cnt = DIVX_LANES >> l, base = divx_level_base(l), below = divx_level_base(l - 1);
        for (unsigned i = tid; i < cnt; i += nt) {
            const mem inv = tree[base + i], left = tree[below + 2 * i], right = tree[below + 2 * i + 1];
            tree[below + 2 * i] = F::mul(inv, right);
            tree[below + 2 * i + 1] = F::mul(inv, left);
        }
        __syncthreads();
    }
    for (unsigned lane = tid; lane < DIVX_LANES; lane += nt) {
        const size_t first = (size_t)blockIdx.x * DIVX_LANES + lane;
        const size_t count = first < slots ? (slots - first + T - 1) / T : 0;
        mem inv = tree[lane];
        for (size_t i = count; i-- > 0; ) {
            const size_t s = first + i * T;
            mem d[V], before[V], q[V];
            lane_split<F, A16, V>(L::load(p.den, V * s, p.n), d);
            // the running product in front of each element: the one parked by the previous element of this slot, or by the last of the previous slot
            lane_split<F, A16, V>(L::load(p.out, V * s, p.n), before);
#pragma unroll
            for (int e = V - 1; e > 0; --e) before[e] = before[e - 1];
            before[0] = i ? F::template load<A16>(p.out, V * (s - T) + (V - 1)) : one;
            typename L::val nm = L::splat(one);
            if (p.num) nm = L::load(p.num, V * s, p.n);
#pragma unroll
            for (int e = V - 1; e >= 0; --e) {
                const bool zero = ops_is_zero<F>(d[e]);
                q[e] = zero ? F::zero() : F::mul(before[e], inv);                                // 1 / d
                if (!zero) inv = F::mul(inv, d[e]);
            }
            typename L::val r = lane_join<F, A16, V>(q);
            if (p.num) r = L::mul(r, nm);
            L::store(p.out, V * s, p.n, r);
        }
    }
}

template<class F, bool A16> __global__ void __launch_bounds__(256) kx_div(DivParamsX<F> p) { div_body<F, A16, false>(p); }
template<class F, bool A16> __global__ void __launch_bounds__(256) kx_div_euclid(DivParamsX<F> p) { div_body<F, A16, true>(p); }

// out[j] = tab[0] + sum_{bit k of j} tab[1 + k]: point - x over a domain (domain_offsets), c - Z_S(x) (vanishing_evals)
template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_subset_sums(uint64_t *out, const uint64_t *tab, int m, size_t n)
{
    typedef LaneX<F, A16> L;
    OPSX_LOOP_V((ops_lane<F, A16>), j, n) L::store(out, j, n, L::sums(tab, m, j));
}

// N = sum_i c_i N_i prod_{k != i} D_k, D = prod_k D_k (rational_linear_combination.tcc:13-108)
#define RATIONALX_MAX 4
template<class F>
struct RationalParamsX {
    const uint64_t *N[RATIONALX_MAX], *D[RATIONALX_MAX];
    typename F::mem c[RATIONALX_MAX];
    uint64_t *outN, *outD;
    int num;
    size_t n;
};

// One rational after the other: with (N, D) the combination of the first i, the next one gives (N D_i + c_i N_i D, D D_i).  Three products per further
// rational (13 at four, against 19 for the sum term by term), and only N, D and the rational at hand are live whatever the number of rationals: no
// array indexed up to a bound of the launch (it would live in scratch memory), no unrolled copies of the body per count.
template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_rational_combine(RationalParamsX<F> p)
{
    typedef LaneX<F, A16> L;
    OPSX_LOOP_V((ops_lane<F, A16>), j, p.n) {
        typename L::val numer = L::mul(L::load(p.N[0], j, p.n), L::splat(p.c[0])), denom = L::load(p.D[0], j, p.n);
#pragma unroll 1
        for (int i = 1; i < p.num; ++i) {
            const typename L::val d = L::load(p.D[i], j, p.n);
            const typename L::val term = L::mul(L::mul(L::load(p.N[i], j, p.n), L::splat(p.c[i])), denom);
            numer = L::add(L::mul(numer, d), term);
            denom = L::mul(denom, d);
        }
        L::store(p.outN, j, p.n, numer);
        L::store(p.outD, j, p.n, denom);
    }
}

// The lean form of the same recurrence for an element of several words (one element per lane): the products of a lane run one after the other
// through ONE product site, a rolled loop whose trip picks its operands by the phase it is in, and every value stays in F::reg form from its load
// (one unpack) to the two stores (one pack each).  Per further rational i the phases are
//   0: t = N_i c_i (and D_i is loaded)    1: t = t D    2: N = N D_i + t    3: D = D D_i
// and the first rational takes phase 0 alone (N = N_0 c_0): 1 + 4 (num - 1) products, the count of the form above.  Live across the site: N, D,
// t, D_i and the two operands, whatever the number of rationals; the phase and the rational's index are uniform over the launch (scalar
// registers, scalar branches).  Field arithmetic is exact, so the outputs are the bytes of the form above.  Which form a field takes by default
// is F::RATIONAL_LEAN, a measurement; the option IOPX_GFX_RATIONAL_FORM overrides it per launch.
template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_rational_combine_lean(RationalParamsX<F> p)
{
    typedef typename F::reg R;
    OPSX_LOOP(j, p.n) {
        R numer = F::unpack(F::zero()), t = numer, d = numer;
        R denom = F::unpack(F::template load<A16>(p.D[0], j));
        int i = 0, phase = 0;
#pragma unroll 1
        while (i < p.num) {
            R a, b;
            if (phase == 0) {
                a = F::unpack(F::template load<A16>(p.N[i], j));
                b = F::unpack(p.c[i]);
                if (i) d = F::unpack(F::template load<A16>(p.D[i], j));
            } else if (phase == 1) {
                a = t; b = denom;
            } else {
                a = phase == 2 ? numer : denom; b = d;
            }
            const R r = F::rmul(a, b);
            if (phase == 0) {
                if (i == 0) { numer = r; i = 1; }
                else { t = r; phase = 1; }
            } else if (phase == 1) {
                t = r; phase = 2;
            } else if (phase == 2) {
                numer = F::unpack(F::add(F::pack(r), F::pack(t))); phase = 3;
            } else {
                denom = r; phase = 0; ++i;
            }
        }
        F::template store<A16>(p.outN, j, F::pack(numer));
        F::template store<A16>(p.outD, j, F::pack(denom));
    }
}

// q(x) = (D(x) (p(x) + eps^-1 mu x^(|K| - 1)) - N(x)) / Z_K(x) (rational_sumcheck.tcc:58-112); x^(|K| - 1) = x^|K| / x with x^|K| a subset sum and
// 1 / x supplied by the caller; Z_K is constant on the cosets of K, the blocks position >> k of the codeword domain: one entry of a table each
template<class F>
struct ConstraintParamsX {
    const uint64_t *p, *N, *D, *xinv;
    const uint64_t *ktab;       // (m + 1)-entry subset-sum table of x^|K|
    const uint64_t *zinv;       // 2^(m - k) entries
    typename F::mem c;          // eps^-1 mu
    uint64_t *out;
    int m, k;
    size_t n;
};

template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_sumcheck_constraint(ConstraintParamsX<F> a)
{
    typedef LaneX<F, A16> L;
    OPSX_LOOP_V((ops_lane<F, A16>), j, a.n) {
        const typename L::operand pp = L::fetch(a.p, j, a.n), nn = L::fetch(a.N, j, a.n), dd = L::fetch(a.D, j, a.n), xi = L::fetch(a.xinv, j, a.n);
        const typename L::cosets z = L::coset(a.zinv, j, a.k, a.n);
        typename L::val s = L::mul(L::mul(L::sums(a.ktab, a.m, j), L::splat(a.c)), L::get(xi, j, a.n));
        s = L::add(s, L::get(pp, j, a.n));
        // characteristic 2: D s - N = D s + N
        const typename L::val t = L::add(L::mul(L::get(dd, j, a.n), s), L::get(nn, j, a.n));
        L::store(a.out, j, a.n, L::mul(t, L::entry(z)));
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
template<class F>
static std::vector<typename F::host> host_elems_x(const uint64_t *w, size_t count)
{
    std::vector<typename F::host> v(count);
    for (size_t i = 0; i < count; ++i) v[i] = typename F::host(w + F::W * i);
    return v;
}

template<class F>
static typename F::mem mem_of_x(const typename F::host &x)
{
    typename F::mem r;
    x.store(reinterpret_cast<uint64_t *>(&r));       // F::mem is F::W words
    return r;
}

template<class F>
static void push_x(std::vector<uint64_t> &v, const typename F::host &x)
{
    uint64_t w[F::W];
    x.store(w);
    v.insert(v.end(), w, w + F::W);
}

// key of a table that depends on two domains of the field: the field's tag and the table's kind keep it apart from every other table of
// runtime.hip's cache
template<class F>
static std::vector<uint64_t> table_key_x(const uint64_t *basis, size_t m, const uint64_t *shift, const uint64_t *sub_basis, size_t sub_dim,
                                         const uint64_t *sub_shift, uint64_t kind)
{
    std::vector<uint64_t> key(basis, basis + F::W * m);
    key.insert(key.end(), shift, shift + F::W);
    if (sub_basis) key.insert(key.end(), sub_basis, sub_basis + F::W * sub_dim);
    key.insert(key.end(), sub_shift, sub_shift + F::W);
    key.push_back(m); key.push_back(sub_dim); key.push_back(F::OPS_TAG); key.push_back(kind);
    return key;
}

// 1 / Z_H on each coset of H = span(basis[0..h)) + constraint_shift inside span(basis[0..m)) + shift (virtual_oracles.hip): evaluated on the
// host, inverted with Montgomery's trick (one field inversion), kept on the device per pair of domains and caller (`kind`; `meets`: the caller's
// refusal of a domain on which Z_H has a zero)
template<class F>
static int vanishing_inverse_table_x(const uint64_t *basis, size_t m, const uint64_t *shift, size_t h, const uint64_t *constraint_shift, TmpBuf &dz,
                                     uint64_t kind = 1, const char *meets = "the codeword domain intersects the constraint domain")
{
    typedef typename F::host H;
    const size_t cosets = (size_t)1 << (m - h);
    return cached_domain_table(table_key_x<F>(basis, m, shift, nullptr, h, constraint_shift, kind), [&](std::vector<uint64_t> &zinv) -> int {
        const std::vector<H> b = host_elems_x<F>(basis, m);
        const SubspacePolyX<H> lin(b.data(), h);
        const H z_shift = lin.eval(H(constraint_shift));
        std::vector<H> z(cosets), prefix(cosets);
        H acc = H::one();
        for (size_t c = 0; c < cosets; ++c) {
            H x(shift);                                         // first element of the coset: index c << h (utils.tcc:8-30)
            for (size_t k = h; k < m; ++k) if ((c >> (k - h)) & 1) x += b[k];
            z[c] = lin.eval(x) + z_shift;
            if (z[c].is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "%s", meets);
            acc = acc * z[c];
            prefix[c] = acc;
        }
        H inv = acc.inverse();
        zinv.resize(F::W * cosets);
        for (size_t c = cosets; c-- > 0;) {
            (c ? inv * prefix[c - 1] : inv).store(&zinv[F::W * c]);
            inv = inv * z[c];
        }
        return IOPX_OK;
    }, dz);
}

template<class F>
struct TermX { size_t off; typename F::host c; };

// the passes of encoded_ops.hip's run_division
template<class F, typename PassTerms>
static int run_division_x(const uint64_t *d_high, size_t M, size_t min_offset, uint64_t *d_quotient, PassTerms terms_of_pass)
{
    // the kernel argument block holds 4 KiB: a division pass has the largest one here
    static_assert(sizeof(PolyDivParamsX<F>) <= 4096, "division pass: argument block too large");
    const size_t EB = 8 * F::W;
    int passes = 0;
    for (size_t o = min_offset; o != 0 && o < M; o <<= 1) ++passes;         // offsets stay below 2 M <= 2^41: no overflow
    if (passes == 0) return d_high != d_quotient ? copy_d2d(d_quotient, d_high, M * EB) : IOPX_OK;
    TmpBuf ping;
    int rc;
    if (passes > 1 && (rc = ping.alloc(M * EB)) != IOPX_OK) return rc;
    const uint64_t *src = d_high;
    for (int k = 0; k < passes; ++k) {
        // the last pass writes the quotient; before that alternate between the temporary and the quotient buffer
        uint64_t *dst = ((passes - 1 - k) & 1) ? ping.u64() : d_quotient;
        PolyDivParamsX<F> p;
        memset(&p, 0, sizeof(p));
        for (const TermX<F> &t : terms_of_pass(k)) {
            if (t.off >= M) continue;
            p.consts[p.nterms] = mem_of_x<F>(t.c);
            p.off[p.nterms++] = t.off;
        }
        if (p.nterms == 0) {        // nothing reaches back into the quotient: the factor is 1 on this range
            if (src != dst && (rc = copy_d2d(dst, src, M * EB)) != IOPX_OK) return rc;
            src = dst;
            continue;
        }
        p.src = src; p.dst = dst; p.M = M;
        IOPX_OPS_LAUNCH(ops_al16(src) && ops_al16(dst), "polydiv_pass", 2 * M * EB, kx_polydiv_pass, 1, M, p);
        IOPX_HIP(hipGetLastError());
        src = dst;
    }
    return IOPX_OK;
}

template<class F>
static int x_add_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (count == 0) return IOPX_OK;
    if (!d_a || !d_b || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    IOPX_OPS_LAUNCH(ops_al16(d_a) && ops_al16(d_b) && ops_al16(d_out), "add", 3 * count * 8 * F::W, kx_add, (ops_lane<F, true>), count, d_out, d_a, d_b, count);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int x_lincomb_dev(const void *const *d_oracles, size_t num, const uint64_t *coeffs, const uint64_t *constant, size_t n, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_oracles || !coeffs || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (num == 0 || num > LINCOMBX_MAX) return fail(IOPX_ERR_INVALID_ARGUMENT, "Random Linear Combination Oracle: Expected same number of evaluations as in registration.");
    LincombParamsX<F> p;
    memset(&p, 0, sizeof(p));
    bool a16 = ops_al16(d_out);
    for (size_t i = 0; i < num; ++i) {
        if (!d_oracles[i]) return fail(IOPX_ERR_INVALID_ARGUMENT, "null oracle");
        p.o[i] = (const uint64_t *)d_oracles[i];
        memcpy(&p.c[i], coeffs + F::W * i, 8 * F::W);
        a16 = a16 && ops_al16(d_oracles[i]);
    }
    if (constant) memcpy(&p.constant, constant, 8 * F::W);
    p.out = d_out; p.num = (int)num; p.n = n;
    if (n == 0) return IOPX_OK;
    IOPX_OPS_LAUNCH(a16, "lincomb", (num + 1) * n * 8 * F::W, kx_lincomb, (ops_lane<F, true>), n, p);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int x_lincomb_affine_dev(const void *const *d_oracles, size_t num, const uint64_t *coeffs, const uint64_t *constant, size_t n, uint64_t *d_out)
{
    if (!constant) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    return x_lincomb_dev<F>(d_oracles, num, coeffs, constant, n, d_out);
}

// d_out[l] = init * base^l for l < count
template<class F>
static int x_pow_table_dev(uint64_t *d_out, size_t count, const uint64_t *base, const uint64_t *init)
{
    typedef typename F::host H;
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_out || !base || !init) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (count == 0) return IOPX_OK;
    PowParamsX<F> p;
    memset(&p, 0, sizeof(p));
    p.nbits = (int)ceil_log2(count);
    if (p.nbits > POWX_MAX_BITS) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension too large");
    H x(base);
    for (int k = 0; k < p.nbits; ++k) { p.sq[k] = mem_of_x<F>(x); x = x.squared(); }
    memcpy(&p.init, init, 8 * F::W);
    IOPX_OPS_LAUNCH(ops_al16(d_out), "pow_table", count * 8 * F::W, kx_pow_table, 1, count, d_out, count, p);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int x_spmv_dev(const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_coeff, size_t rows, const uint64_t *d_vec,
                      const uint64_t *scale, int accumulate, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (rows == 0) return IOPX_OK;
    if (!d_row_ptr || !d_col || !d_coeff || !d_vec || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    SpmvParamsX<F> p;
    memset(&p, 0, sizeof(p));
    p.row_ptr = d_row_ptr; p.col = d_col; p.coeff = d_coeff; p.vec = d_vec; p.out = d_out; p.rows = rows; p.accumulate = accumulate;
    p.has_scale = scale ? 1 : 0;
    if (scale) memcpy(&p.scale, scale, 8 * F::W);
    // the entries are counted on the device only: the rows' output is what the host can declare
    IOPX_OPS_LAUNCH(ops_al16(d_coeff) && ops_al16(d_vec) && ops_al16(d_out), "spmv", (size_t)(accumulate ? 2 : 1) * rows * 8 * F::W, kx_spmv, 1, rows, p);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int x_lincheck_dev(const uint64_t *d_fz, const void *const *d_Mz, size_t num_matrices, const uint64_t *r_Mz,
                          const uint64_t *d_p_alpha_prime, const uint64_t *d_p_alpha_ABC, size_t n, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_fz || !d_Mz || !r_Mz || !d_p_alpha_prime || !d_p_alpha_ABC || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (num_matrices == 0 || num_matrices > LINCHECKX_MAX_MATRICES)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "multi_lincheck uses more constituent oracles than what was provided.");
    LincheckParamsX<F> p;
    memset(&p, 0, sizeof(p));
    p.fz = d_fz; p.p1 = d_p_alpha_prime; p.p2 = d_p_alpha_ABC; p.out = d_out;
    bool a16 = ops_al16(d_fz) && ops_al16(d_p_alpha_prime) && ops_al16(d_p_alpha_ABC) && ops_al16(d_out);
    for (size_t m = 0; m < num_matrices; ++m) {
        if (!d_Mz[m]) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
        p.mz[m] = (const uint64_t *)d_Mz[m];
        memcpy(&p.r[m], r_Mz + F::W * m, 8 * F::W);
        a16 = a16 && ops_al16(d_Mz[m]);
    }
    p.num_matrices = (int)num_matrices; p.n = n;
    if (n == 0) return IOPX_OK;
    IOPX_OPS_LAUNCH(a16, "lincheck", (num_matrices + 4) * n * 8 * F::W, kx_lincheck, (ops_lane<F, true>), n, p);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int x_rowcheck_dev(const uint64_t *d_Az, const uint64_t *d_Bz, const uint64_t *d_Cz, const uint64_t *basis, size_t m,
                          const uint64_t *shift, size_t constraint_dim, const uint64_t *constraint_shift, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_Az || !d_Bz || !d_Cz || !d_out || (m > 0 && !basis) || !shift || !constraint_shift) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (constraint_dim > m || m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "the constraint domain must be a sub-domain of the codeword domain");
    const size_t h = constraint_dim;
    TmpBuf dz;
    if ((rc = vanishing_inverse_table_x<F>(basis, m, shift, h, constraint_shift, dz)) != IOPX_OK) return rc;
    const size_t n = (size_t)1 << m;
    IOPX_OPS_LAUNCH(ops_al16(d_Az) && ops_al16(d_Bz) && ops_al16(d_Cz) && ops_al16(d_out) && ops_table_al16<F>(dz.p), "rowcheck", 4 * n * 8 * F::W,
                    kx_rowcheck, (ops_lane<F, true>), n, d_out, d_Az, d_Bz, d_Cz, (const uint64_t *)dz.u64(), (int)h, n);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int x_fz_dev(const uint64_t *d_fw, const uint64_t *d_f1v, const uint64_t *basis, size_t m, const uint64_t *shift,
                    const uint64_t *input_basis, size_t input_dim, const uint64_t *input_shift, uint64_t *d_out)
{
    typedef typename F::host H;
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_fw || !d_f1v || !d_out || (m > 0 && !basis) || !shift || (input_dim > 0 && !input_basis) || !input_shift)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (input_dim > m || m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "Codeword domain must be bigger than the input variable domain.");
    // the subset-sum table of Z_I over the codeword domain: a function of the two domains only, kept on the device
    TmpBuf dt;
    rc = cached_domain_table(table_key_x<F>(basis, m, shift, input_basis, input_dim, input_shift, 2), [&](std::vector<uint64_t> &tab) -> int {
        const std::vector<H> ib = host_elems_x<F>(input_basis, input_dim);
        const SubspacePolyX<H> lin(ib.data(), input_dim);                                  // Z_I's linear part
        push_x<F>(tab, lin.eval(H(shift)) + lin.eval(H(input_shift)));                     // Z_I(shift) = lin(shift) + lin(shift_I)
        for (size_t k = 0; k < m; ++k) push_x<F>(tab, lin.eval(H(basis + F::W * k)));
        return IOPX_OK;
    }, dt);
    if (rc != IOPX_OK) return rc;
    const size_t n = (size_t)1 << m;
    IOPX_OPS_LAUNCH(ops_al16(d_fw) && ops_al16(d_f1v) && ops_al16(d_out) && ops_table_al16<F>(dt.p), "fz", 3 * n * 8 * F::W, kx_fz, (ops_lane<F, true>), n,
                    d_out, d_fw, d_f1v, (const uint64_t *)dt.u64(), (int)m, n);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int x_sumcheck_g_dev(const uint64_t *d_f, const uint64_t *d_h, const uint64_t *basis, size_t m, const uint64_t *shift,
                            const uint64_t *summation_basis, size_t summation_dim, const uint64_t *summation_shift,
                            const uint64_t *claimed_sum, uint64_t *d_out)
{
    typedef typename F::host H;
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_f || !d_h || !d_out || (m > 0 && !basis) || !shift || (summation_dim > 0 && !summation_basis) || !summation_shift || !claimed_sum)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (m > 40 || summation_dim > 63) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension too large");
    const std::vector<H> sb = host_elems_x<F>(summation_basis, summation_dim);
    const SubspacePolyX<H> lin(sb.data(), summation_dim);                                  // Z_H's linear part
    if (lin.coeff[0].is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "the summation domain's basis is linearly dependent");
    const H c = lin.coeff[0].inverse() * H(claimed_sum);                                   // eps^-1 mu (sumcheck.tcc:52-54)
    // the subset-sum tables of x, x^|H| and Z_H(x) over the codeword domain: functions of the two domains only, kept on the device (one block)
    const size_t table_words = F::W * (m + 1);
    TmpBuf dtabs;
    rc = cached_domain_table(table_key_x<F>(basis, m, shift, summation_basis, summation_dim, summation_shift, 3), [&](std::vector<uint64_t> &words) -> int {
        words.assign(3 * table_words, 0);
        for (size_t k = 0; k <= m; ++k) {
            const H v(k == 0 ? shift : basis + F::W * (k - 1));
            H vh = v;
            for (size_t i = 0; i < summation_dim; ++i) vh = vh.squared();                  // v^|H|
            H vz = lin.eval(v);
            if (k == 0) vz += lin.eval(H(summation_shift));                                // Z_H(shift) = lin(shift) + lin(shift_H)
            v.store(&words[F::W * k]); vh.store(&words[table_words + F::W * k]); vz.store(&words[2 * table_words + F::W * k]);
        }
        return IOPX_OK;
    }, dtabs);
    if (rc != IOPX_OK) return rc;
    SumcheckParamsX<F> p;
    memset(&p, 0, sizeof(p));
    p.f = d_f; p.h = d_h; p.out = d_out;
    p.xtab = dtabs.u64(); p.htab = dtabs.u64() + table_words; p.ztab = dtabs.u64() + 2 * table_words;
    p.c = mem_of_x<F>(c); p.m = (int)m; p.n = (size_t)1 << m;
    // the three tables are whole elements apart: where an element is 16 bytes or more they are aligned together with the block
    const bool a16 = ops_al16(d_f) && ops_al16(d_h) && ops_al16(d_out) && ops_table_al16<F>(p.xtab) && ops_table_al16<F>(p.htab) && ops_table_al16<F>(p.ztab);
    if (c.is_zero()) IOPX_OPS_LAUNCH(a16, "sumcheck_g_zero_sum", 3 * p.n * 8 * F::W, kx_sumcheck_g_zero_sum, (ops_lane<F, true>), p.n, p);
    else IOPX_OPS_LAUNCH(a16, "sumcheck_g", 3 * p.n * 8 * F::W, kx_sumcheck_g, (ops_lane<F, true>), p.n, p);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int x_poly_div_vanishing_dev(const uint64_t *d_poly, size_t n_coeffs, const uint64_t *basis, size_t dim, const uint64_t *shift,
                                    uint64_t *d_quotient)
{
    typedef typename F::host H;
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_poly || (dim > 0 && !basis) || !shift || !d_quotient) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (dim > 62) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension too large");
    const size_t N = (size_t)1 << dim;
    if (n_coeffs <= N) return IOPX_OK;                       // empty quotient (linearized_polynomial.tcc:247-255)
    const size_t M = n_coeffs - N;
    // Z = sum_{i <= dim} lin[i] X^(2^i) + lin(shift) (vanishing_polynomial.tcc:373-395)
    const std::vector<H> b = host_elems_x<F>(basis, dim);
    const SubspacePolyX<H> lin(b.data(), dim);
    if (!(lin.coeff[dim] == H::one())) return fail(IOPX_ERR_LOGIC, "vanishing polynomial is not monic");
    const H c_const = lin.eval(H(shift));
    std::vector<H> cur;                                      // c_i^(2^k), squared once per pass
    std::vector<size_t> base_off;
    for (size_t i = 0; i < dim; ++i) if (!lin.coeff[i].is_zero()) { cur.push_back(lin.coeff[i]); base_off.push_back(N - ((size_t)1 << i)); }
    if (!c_const.is_zero()) { cur.push_back(c_const); base_off.push_back(N); }
    if (cur.size() > PDIVX_MAX_TERMS) return fail(IOPX_ERR_INVALID_ARGUMENT, "too many terms");
    size_t min_off = 0;
    for (size_t o : base_off) if (min_off == 0 || o < min_off) min_off = o;
    int done = 0;
    auto terms_of_pass = [&](int k) {
        while (done < k) { for (H &c : cur) c = c.squared(); ++done; }
        std::vector<TermX<F>> t;
        for (size_t i = 0; i < cur.size(); ++i) {
            TermX<F> x;
            x.off = base_off[i] << k;
            x.c = cur[i];
            t.push_back(x);
        }
        return t;
    };
    return run_division_x<F>(d_poly + F::W * N, M, min_off, d_quotient, terms_of_pass);
}

// d_out[j] = d_in[j] / Z_S(x_j) over span(basis[0..m)) + shift, S = span(basis[0..sub_dim)) + sub_shift (d_out may be d_in)
template<class F>
static int x_div_by_vanishing_dev(const uint64_t *d_in, const uint64_t *basis, size_t m, const uint64_t *shift, size_t sub_dim, const uint64_t *sub_shift,
                                  uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_in || !d_out || (m > 0 && !basis) || !shift || !sub_shift) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (sub_dim > m || m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "the vanishing set must be spanned by a prefix of the domain's basis");
    TmpBuf dz;
    if ((rc = vanishing_inverse_table_x<F>(basis, m, shift, sub_dim, sub_shift, dz, 4, "the domain intersects the vanishing set")) != IOPX_OK) return rc;
    const size_t n = (size_t)1 << m;
    IOPX_OPS_LAUNCH(ops_al16(d_in) && ops_al16(d_out) && ops_table_al16<F>(dz.p), "div_by_vanishing", 2 * n * 8 * F::W, kx_div_by_vanishing,
                    (ops_lane<F, true>), n, d_out, d_in, (const uint64_t *)dz.u64(), (int)sub_dim, n);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

// Z_S(x) and Z_S's linear coefficient (its formal derivative, vanishing_polynomial.tcc:55-74) for S = span(basis) + shift: host only
template<class F>
static int x_vanishing_host(const uint64_t *basis, size_t dim, const uint64_t *shift, const uint64_t *x, uint64_t *value_out, uint64_t *linear_coefficient_out)
{
    typedef typename F::host H;
    if ((dim > 0 && !basis) || !shift || !x) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (dim > 63) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension too large");
    const std::vector<H> b = host_elems_x<F>(basis, dim);
    const SubspacePolyX<H> lin(b.data(), dim);
    if (value_out) (lin.eval(H(x)) + lin.eval(H(shift))).store(value_out);
    if (linear_coefficient_out) lin.coeff[0].store(linear_coefficient_out);
    return IOPX_OK;
}

// ---- the holographic prover's entries: the arguments, refusals and messages of the gf192 entries of fractal_ops.hip ----------------------------
// 16 slots per lane while that fills the GPU (the shared inversion is one lane's serial work per workgroup), 2048 workgroups at most
static int div_grid_x(size_t slots)
{
    size_t cap = (size_t)opt_range("IOPX_GFX_OPS_MAX_BLOCKS", 16384, 1, 16384);
    if (cap > DIVX_MAX_BLOCKS) cap = DIVX_MAX_BLOCKS;
    size_t g = (slots + DIVX_LANES * DIVX_SLOTS_PER_LANE - 1) / (DIVX_LANES * DIVX_SLOTS_PER_LANE);
    if (g > cap) g = cap;
    return (int)(g ? g : 1);
}

template<class F>
static int x_div_dev(const uint64_t *d_num, const uint64_t *d_den, uint64_t *d_out, size_t n)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (n == 0) return IOPX_OK;
    if (!d_den || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (d_out == d_den || d_out == d_num) return fail(IOPX_ERR_INVALID_ARGUMENT, "the quotient buffer holds the running products: it cannot alias an input");
    DivParamsX<F> p;
    p.num = d_num; p.den = d_den; p.out = d_out; p.n = n;
    // den read twice, out written twice and read once (, num read once).  The root's inversion: the field's measured choice (F::DIV_EUCLID, DESIGN.md
    // §5.18), or what the option IOPX_GFX_DIV_INVERSION asks for (1: the Fermat power, 2: Euclid; a measuring and test helper, looked up per launch)
    const int inversion = opt_range("IOPX_GFX_DIV_INVERSION", 0, 0, 2);
    const bool a16 = ops_al16(d_den) && ops_al16(d_out) && (!d_num || ops_al16(d_num));
    const size_t bytes = n * 8 * F::W * (d_num ? 6 : 5), lds = (size_t)DIVX_TREE_NODES * 8 * F::W + 8;
    if (inversion ? inversion == 2 : F::DIV_EUCLID) IOPX_OPS_LAUNCH_ON(a16, "div", bytes, kx_div_euclid, (ops_lane<F, true>), n, div_grid_x, lds, p);
    else IOPX_OPS_LAUNCH_ON(a16, "div", bytes, kx_div, (ops_lane<F, true>), n, div_grid_x, lds, p);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

// d_out[j] = tab[0] + the subset sum of tab[1..m] over the bits of j; tab: the (m + 1) entries of a launch, uploaded (a domain of dimension 40
// has 41: too many for the argument block at four words beside nothing else, and a table costs one small copy)
template<class F, bool OFFSETS>
static int subset_sums_x(const std::vector<uint64_t> &tab, size_t m, uint64_t *d_out)
{
    int rc;
    TmpBuf dt;
    if ((rc = dt.alloc(tab.size() * 8)) != IOPX_OK) return rc;
    if ((rc = upload(dt.p, tab.data(), tab.size() * 8)) != IOPX_OK) return rc;
    const size_t n = (size_t)1 << m;
    // one kernel under the name of its caller (a launch site builds its profile names once)
    if (OFFSETS) IOPX_OPS_LAUNCH(ops_al16(d_out) && ops_table_al16<F>(dt.p), "domain_offsets", n * 8 * F::W, kx_subset_sums, (ops_lane<F, true>), n, d_out, (const uint64_t *)dt.u64(), (int)m, n);
    else IOPX_OPS_LAUNCH(ops_al16(d_out) && ops_table_al16<F>(dt.p), "vanishing_evals", n * 8 * F::W, kx_subset_sums, (ops_lane<F, true>), n, d_out, (const uint64_t *)dt.u64(), (int)m, n);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

// d_out[j] = point - x_j over span(basis[0..m)) + shift
template<class F>
static int x_domain_offsets_dev(const uint64_t *basis, size_t m, const uint64_t *shift, const uint64_t *point, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if ((m > 0 && !basis) || !shift || !point || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension too large");
    std::vector<uint64_t> tab(F::W * (m + 1));
    for (int w = 0; w < F::W; ++w) tab[w] = shift[w] ^ point[w];               // point - x = point + shift + sum of basis vectors
    if (m) memcpy(&tab[F::W], basis, 8 * F::W * m);
    return subset_sums_x<F, true>(tab, m, d_out);
}

// d_out[j] = constant - Z_S(x_j) over span(basis[0..m)) + shift, S = span(vanishing_basis) + vanishing_shift
template<class F>
static int x_vanishing_evals_dev(const uint64_t *basis, size_t m, const uint64_t *shift, const uint64_t *vanishing_basis, size_t vanishing_dim,
                                 const uint64_t *vanishing_shift, const uint64_t *constant, uint64_t *d_out)
{
    typedef typename F::host H;
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if ((m > 0 && !basis) || !shift || (vanishing_dim > 0 && !vanishing_basis) || !vanishing_shift || !constant || !d_out)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (m > 40 || vanishing_dim > 63) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension too large");
    const std::vector<H> vb = host_elems_x<F>(vanishing_basis, vanishing_dim);
    const SubspacePolyX<H> lin(vb.data(), vanishing_dim);
    std::vector<uint64_t> tab;
    push_x<F>(tab, H(constant) + lin.eval(H(shift)) + lin.eval(H(vanishing_shift)));
    for (size_t k = 0; k < m; ++k) push_x<F>(tab, lin.eval(H(basis + F::W * k)));
    return subset_sums_x<F, false>(tab, m, d_out);
}

template<class F>
static int x_rational_combine_dev(const void *const *d_N, const void *const *d_D, size_t num, const uint64_t *coeffs, size_t n, uint64_t *d_outN,
                                  uint64_t *d_outD)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_N || !d_D || !coeffs || !d_outN || !d_outD) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (num == 0 || num > RATIONALX_MAX) return fail(IOPX_ERR_INVALID_ARGUMENT, "Expected same number of evaluations as in registration.");
    RationalParamsX<F> p;
    memset(&p, 0, sizeof(p));
    bool a16 = ops_al16(d_outN) && ops_al16(d_outD);
    for (size_t i = 0; i < num; ++i) {
        if (!d_N[i] || !d_D[i]) return fail(IOPX_ERR_INVALID_ARGUMENT, "null oracle");
        p.N[i] = (const uint64_t *)d_N[i]; p.D[i] = (const uint64_t *)d_D[i];
        memcpy(&p.c[i], coeffs + F::W * i, 8 * F::W);
        a16 = a16 && ops_al16(d_N[i]) && ops_al16(d_D[i]);
    }
    p.outN = d_outN; p.outD = d_outD; p.num = (int)num; p.n = n;
    if (n == 0) return IOPX_OK;
    // The form: the field's measured choice (F::RATIONAL_LEAN), or what the option IOPX_GFX_RATIONAL_FORM asks for (1: one rational
    // after the other with inlined products, 2: the lean form; a measuring and test helper, looked up per launch).  The lean form exists for an
    // element of several words; over a one-word element every value of the option gives the one form there is.
    const int form = opt_range("IOPX_GFX_RATIONAL_FORM", 0, 0, 2);
    bool lean = false;
    if constexpr (F::W > 1) lean = form ? form == 2 : F::RATIONAL_LEAN;
    if constexpr (F::W > 1) {
        if (lean) IOPX_OPS_LAUNCH(a16, "rational_combine", n * 8 * F::W * (2 * num + 2), kx_rational_combine_lean, 1, n, p);
    }
    if (!lean) IOPX_OPS_LAUNCH(a16, "rational_combine", n * 8 * F::W * (2 * num + 2), kx_rational_combine, (ops_lane<F, true>), n, p);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int x_rational_sumcheck_constraint_dev(const uint64_t *d_p, const uint64_t *d_N, const uint64_t *d_D, const uint64_t *d_xinv, const uint64_t *basis,
                                              size_t m, const uint64_t *shift, size_t summation_dim, const uint64_t *summation_shift,
                                              const uint64_t *claimed_sum, uint64_t *d_out)
{
    typedef typename F::host H;
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_p || !d_N || !d_D || !d_xinv || !d_out || (m > 0 && !basis) || !shift || !summation_shift || !claimed_sum)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (summation_dim > m || m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "the summation domain must be spanned by a prefix of the codeword domain's basis");
    const size_t k = summation_dim;
    const std::vector<H> kb = host_elems_x<F>(basis, k);
    const SubspacePolyX<H> lin(kb.data(), k);
    if (lin.coeff[0].is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "the summation domain's basis is linearly dependent");
    const H c = lin.coeff[0].inverse() * H(claimed_sum);                                   // eps^-1 mu (rational_sumcheck.tcc:52-56)
    // 1 / Z_K per coset of K, and the subset-sum table of x^|K| over the codeword domain: functions of the two domains only, kept on the device
    TmpBuf dz, dk;
    if ((rc = vanishing_inverse_table_x<F>(basis, m, shift, k, summation_shift, dz, 5, "the codeword domain intersects the summation domain")) != IOPX_OK) return rc;
    rc = cached_domain_table(table_key_x<F>(basis, m, shift, nullptr, k, summation_shift, 6), [&](std::vector<uint64_t> &tab) -> int {
        for (size_t i = 0; i <= m; ++i) {
            H v(i == 0 ? shift : basis + F::W * (i - 1));
            for (size_t s = 0; s < k; ++s) v = v.squared();                                // v^|K|
            push_x<F>(tab, v);
        }
        return IOPX_OK;
    }, dk);
    if (rc != IOPX_OK) return rc;
    ConstraintParamsX<F> a;
    memset(&a, 0, sizeof(a));
    a.p = d_p; a.N = d_N; a.D = d_D; a.xinv = d_xinv; a.ktab = dk.u64(); a.zinv = dz.u64(); a.c = mem_of_x<F>(c); a.out = d_out;
    a.m = (int)m; a.k = (int)k; a.n = (size_t)1 << m;
    IOPX_OPS_LAUNCH(ops_al16(d_p) && ops_al16(d_N) && ops_al16(d_D) && ops_al16(d_xinv) && ops_al16(d_out) && ops_table_al16<F>(dk.p) && ops_table_al16<F>(dz.p),
                    "rational_sumcheck_constraint", a.n * 8 * F::W * 5, kx_sumcheck_constraint, (ops_lane<F, true>), a.n, a);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

} // namespace iopx

// the C entries of one field: iopx_*_<field>_dev over the bodies above
#define IOPX_GFX_OPS_ENTRIES(FIELD, F)                                                                                                                          \
    extern "C" {                                                                                                                                                \
    int iopx_##FIELD##_add_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count)                                                         \
    {                                                                                                                                                           \
        return iopx::x_add_dev<F>(d_a, d_b, d_out, count);                                                                                                      \
    }                                                                                                                                                           \
    int iopx_##FIELD##_pow_table_dev(uint64_t *d_out, size_t count, const uint64_t *base, const uint64_t *init)                                                 \
    {                                                                                                                                                           \
        return iopx::x_pow_table_dev<F>(d_out, count, base, init);                                                                                              \
    }                                                                                                                                                           \
    int iopx_lincomb_##FIELD##_dev(const void *const *d_oracles, size_t num_oracles, const uint64_t *coefficients, size_t n, uint64_t *d_out)                   \
    {                                                                                                                                                           \
        return iopx::x_lincomb_dev<F>(d_oracles, num_oracles, coefficients, nullptr, n, d_out);                                                                 \
    }                                                                                                                                                           \
    int iopx_lincomb_affine_##FIELD##_dev(const void *const *d_oracles, size_t num_oracles, const uint64_t *coefficients, const uint64_t *constant, size_t n,   \
                                          uint64_t *d_out)                                                                                                      \
    {                                                                                                                                                           \
        return iopx::x_lincomb_affine_dev<F>(d_oracles, num_oracles, coefficients, constant, n, d_out);                                                         \
    }                                                                                                                                                           \
    int iopx_spmv_##FIELD##_dev(const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_coeff, size_t rows, const uint64_t *d_vec,                  \
                                const uint64_t *scale, int accumulate, uint64_t *d_out)                                                                         \
    {                                                                                                                                                           \
        return iopx::x_spmv_dev<F>(d_row_ptr, d_col, d_coeff, rows, d_vec, scale, accumulate, d_out);                                                           \
    }                                                                                                                                                           \
    int iopx_lincheck_##FIELD##_dev(const uint64_t *d_fz, const void *const *d_Mz, size_t num_matrices, const uint64_t *r_Mz,                                   \
                                    const uint64_t *d_p_alpha_prime, const uint64_t *d_p_alpha_ABC, size_t n, uint64_t *d_out)                                  \
    {                                                                                                                                                           \
        return iopx::x_lincheck_dev<F>(d_fz, d_Mz, num_matrices, r_Mz, d_p_alpha_prime, d_p_alpha_ABC, n, d_out);                                               \
    }                                                                                                                                                           \
    int iopx_rowcheck_##FIELD##_dev(const uint64_t *d_Az, const uint64_t *d_Bz, const uint64_t *d_Cz, const uint64_t *basis, size_t m,                          \
                                    const uint64_t *shift, size_t constraint_dim, const uint64_t *constraint_shift, uint64_t *d_out)                            \
    {                                                                                                                                                           \
        return iopx::x_rowcheck_dev<F>(d_Az, d_Bz, d_Cz, basis, m, shift, constraint_dim, constraint_shift, d_out);                                             \
    }                                                                                                                                                           \
    int iopx_fz_##FIELD##_dev(const uint64_t *d_fw, const uint64_t *d_f1v, const uint64_t *basis, size_t m, const uint64_t *shift,                              \
                              const uint64_t *input_basis, size_t input_dim, const uint64_t *input_shift, uint64_t *d_out)                                      \
    {                                                                                                                                                           \
        return iopx::x_fz_dev<F>(d_fw, d_f1v, basis, m, shift, input_basis, input_dim, input_shift, d_out);                                                     \
    }                                                                                                                                                           \
    int iopx_sumcheck_g_##FIELD##_dev(const uint64_t *d_f, const uint64_t *d_h, const uint64_t *basis, size_t m, const uint64_t *shift,                         \
                                      const uint64_t *summation_basis, size_t summation_dim, const uint64_t *summation_shift,                                   \
                                      const uint64_t *claimed_sum, uint64_t *d_out)                                                                             \
    {                                                                                                                                                           \
        return iopx::x_sumcheck_g_dev<F>(d_f, d_h, basis, m, shift, summation_basis, summation_dim, summation_shift, claimed_sum, d_out);                       \
    }                                                                                                                                                           \
    int iopx_poly_div_vanishing_##FIELD##_dev(const uint64_t *d_poly, size_t n_coeffs, const uint64_t *basis, size_t dim, const uint64_t *shift,                \
                                              uint64_t *d_quotient)                                                                                             \
    {                                                                                                                                                           \
        return iopx::x_poly_div_vanishing_dev<F>(d_poly, n_coeffs, basis, dim, shift, d_quotient);                                                              \
    }                                                                                                                                                           \
    int iopx_div_by_vanishing_##FIELD##_dev(const uint64_t *d_in, const uint64_t *basis, size_t m, const uint64_t *shift, size_t sub_dim,                      \
                                            const uint64_t *sub_shift, uint64_t *d_out)                                                                         \
    {                                                                                                                                                           \
        return iopx::x_div_by_vanishing_dev<F>(d_in, basis, m, shift, sub_dim, sub_shift, d_out);                                                               \
    }                                                                                                                                                           \
    int iopx_##FIELD##_vanishing_host(const uint64_t *basis, size_t dim, const uint64_t *shift, const uint64_t *x, uint64_t *value_out,                         \
                                      uint64_t *linear_coefficient_out)                                                                                         \
    {                                                                                                                                                           \
        return iopx::x_vanishing_host<F>(basis, dim, shift, x, value_out, linear_coefficient_out);                                                              \
    }                                                                                                                                                           \
    int iopx_##FIELD##_div_dev(const uint64_t *d_num, const uint64_t *d_den, uint64_t *d_out, size_t count)                                                     \
    {                                                                                                                                                           \
        return iopx::x_div_dev<F>(d_num, d_den, d_out, count);                                                                                                  \
    }                                                                                                                                                           \
    int iopx_domain_offsets_##FIELD##_dev(const uint64_t *basis, size_t m, const uint64_t *shift, const uint64_t *point, uint64_t *d_out)                       \
    {                                                                                                                                                           \
        return iopx::x_domain_offsets_dev<F>(basis, m, shift, point, d_out);                                                                                    \
    }                                                                                                                                                           \
    int iopx_vanishing_evals_##FIELD##_dev(const uint64_t *basis, size_t m, const uint64_t *shift, const uint64_t *vanishing_basis, size_t vanishing_dim,       \
                                           const uint64_t *vanishing_shift, const uint64_t *constant, uint64_t *d_out)                                          \
    {                                                                                                                                                           \
        return iopx::x_vanishing_evals_dev<F>(basis, m, shift, vanishing_basis, vanishing_dim, vanishing_shift, constant, d_out);                               \
    }                                                                                                                                                           \
    int iopx_rational_combine_##FIELD##_dev(const void *const *d_numerators, const void *const *d_denominators, size_t num_rationals,                           \
                                            const uint64_t *coefficients, size_t n, uint64_t *d_numerator_out, uint64_t *d_denominator_out)                     \
    {                                                                                                                                                           \
        return iopx::x_rational_combine_dev<F>(d_numerators, d_denominators, num_rationals, coefficients, n, d_numerator_out, d_denominator_out);               \
    }                                                                                                                                                           \
    int iopx_rational_sumcheck_constraint_##FIELD##_dev(const uint64_t *d_p, const uint64_t *d_N, const uint64_t *d_D, const uint64_t *d_xinv,                  \
                                                        const uint64_t *basis, size_t m, const uint64_t *shift, size_t summation_dim,                           \
                                                        const uint64_t *summation_shift, const uint64_t *claimed_sum, uint64_t *d_out)                          \
    {                                                                                                                                                           \
        return iopx::x_rational_sumcheck_constraint_dev<F>(d_p, d_N, d_D, d_xinv, basis, m, shift, summation_dim, summation_shift, claimed_sum, d_out);         \
    }                                                                                                                                                           \
    }
