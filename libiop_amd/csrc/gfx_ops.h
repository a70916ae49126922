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
//
// Every kernel reads each input once and writes the output once, in a grid-stride loop.  An element travels as F::mem through F::load<A16> /
// F::store<A16>: the A16 instantiation (16-byte accesses) runs when every device pointer that it reads or writes 16 bytes at a time is 16-byte
// aligned, the other one (64-bit words, "_w64" in the profile) otherwise.  A lane takes one element; in the 16-byte form over a one-word
// element it takes the two consecutive elements of one access (ops_lane) where the position of an element does not enter the addressing
// beyond "j and j + 1": everywhere but the powers of a base, the CSR gather and the division passes (odd offsets), which have one form over
// such an element and the plain name.  Constants of a launch (coefficients, the squares of a base, the terms of a division pass) travel in
// the kernel's argument block: no upload.  The domain-shaped values Z_I(x_j), Z_H(x_j), x_j, x_j^|H| are subset sums of an (m + 1)-entry
// table over the bits of j (linearized_polynomial.tcc:83-108); position j + 1 of a pair differs from position j by the table's entry for
// bit 0.  No LDS.  The grid is capped by the option IOPX_GFX_OPS_MAX_BLOCKS (default 16384, looked up per launch; a test helper: a small cap
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
#define IOPX_OPS_LAUNCH(a16, name, bytes, K, lane, work, ...)                                                          \
    do {                                                                                                               \
        constexpr size_t lane_ = (lane);                                                                               \
        constexpr bool forms_ = F::W > 1 || lane_ > 1;                                                                 \
        const bool a16_ = forms_ && (a16);                                                                             \
        static const std::string names_[2] = { std::string(F::stem()) + name, std::string(F::stem()) + name + "_w64" }; \
        ProfScope ps_(names_[forms_ && !a16_ ? 1 : 0].c_str(), bytes);                                                 \
        const dim3 grid_(ops_grid_x(a16_ ? ((work) + lane_ - 1) / lane_ : (work)));                                    \
        if constexpr (forms_) {                                                                                        \
            if (a16_) hipLaunchKernelGGL((K<F, true>), grid_, dim3(256), 0, stream(), __VA_ARGS__);                    \
            else hipLaunchKernelGGL((K<F, false>), grid_, dim3(256), 0, stream(), __VA_ARGS__);                        \
        } else {                                                                                                       \
            hipLaunchKernelGGL((K<F, false>), grid_, dim3(256), 0, stream(), __VA_ARGS__);                             \
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
    }
