// The vector-sized steps of the encoded Aurora prover that are not transforms or virtual oracles, on gfx950:
//
//   iopx_spmv_*                  r1cs_constraint_system::create_Az_Bz_Cz_from_variable_assignment (libiop/relations/r1cs.tcc:236-268)
//                                and the p_alpha_ABC accumulation of multi_lincheck_virtual_oracle::set_challenge
//                                (libiop/protocols/encoded/lincheck/basic_lincheck_aux.tcc:64-88), both as CSR row gathers
//   iopx_poly_div_vanishing_*    polynomial_over_vanishing_polynomial(...).first (libiop/algebra/polynomials/
//                                vanishing_polynomial.tcc:314-371, linearized_polynomial.tcc:238-289): f_w = f_w' / Z_I
//                                (r1cs_rs_iop.tcc:563-565) and the sumcheck's h = f / Z_H (sumcheck.tcc:359-365)
//   iopx_lincomb_*               random_linear_combination_oracle::evaluated_contents (encoded/common/random_linear_combination.tcc:27-57)
//   iopx_*_{add,sub,mul,inv}_dev elementwise field helpers (the synthetic-instance generator r1cs_examples.tcc:40-64, f_w' = z - f_1v)
//
// Division without the reference's serial sweep.  With n coefficients, N = deg Z and M = n - N quotient coefficients, reversing
// the polynomials turns P = Q Z + R into rev(Q) = rev(P) / rev(Z) mod Y^M, rev(Z) = 1 + u(Y) with u sparse:
//   subspaces: u = sum_i c_i Y^(N - 2^i) (+ c_const Y^N),   cosets: u = -c Y^N.
// (1 + u)^-1 = prod_k (1 + u^(2^k)) in characteristic 2 (Frobenius keeps u^(2^k) as sparse as u); (1 - x)^-1 = prod_k (1 + x^(2^k))
// in any field.  Each factor is one data-parallel pass Q[j] += sum_t const_t * Q[j + offset_t]; the offsets double per pass, so
// log2(M / (N/2)) passes suffice (one pass for the sumcheck's h, where deg f < 2 |H|).  Quotients are unique: same bytes.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "gf192_dev.h"
#include "gf192_host.h"
#include "fp3_dev.h"
#include "fp3_host.h"
#include "bn254_dev.h"
#include "mul_field.h"
#include "runtime.h"

namespace iopx {

static int eo_grid(size_t n)
{
    size_t g = (n + 255) / 256;
    if (g > 16384) g = 16384;
    return (int)(g ? g : 1);
}

// ---- elementwise ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gf192_add(uint64_t *out, const uint64_t *a, const uint64_t *b, size_t n)
{
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x)
        gf_store(out, j, gf_add(gf_load(a, j), gf_load(b, j)));
}

__global__ void __launch_bounds__(256) k_gf192_inv(uint64_t *out, const uint64_t *a, size_t n)
{
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) {
        const gf192 x = gf_load(a, j);
        gf_store(out, j, gf_is_zero(x) ? x : gf_inv(x));
    }
}

// F_p: the device product is a b 2^-203 (fp3_dev.h).  Data live as x 2^192 (libff), so data x data = x y 2^181 and one more
// product with the raw constant 2^214 restores libff's form; consts[0] = 2^214, consts[1] = 2^192 (raw words).
__global__ void __launch_bounds__(256) k_fp3_mul(uint64_t *out, const uint64_t *a, const uint64_t *b, const uint64_t *consts, size_t n)
{
    const fp3 k214 = fp_load(consts, 0);
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x)
        fp_store(out, j, fp_mul(fp_mul(fp_load(a, j), fp_load(b, j)), k214));
}

__global__ void __launch_bounds__(256) k_fp3_sub(uint64_t *out, const uint64_t *a, const uint64_t *b, size_t n)
{
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x)
        fp_store(out, j, fp_sub(fp_load(a, j), fp_load(b, j)));
}

// x^(p-2) in the 2^203 form (closed under fp_mul), exponent bits in consts[2] (three raw words), back to libff's form at the end
__global__ void __launch_bounds__(256) k_fp3_inv(uint64_t *out, const uint64_t *a, const uint64_t *consts, size_t n)
{
    const fp3 k214 = fp_load(consts, 0), k192 = fp_load(consts, 1);
    const uint64_t e0 = consts[6], e1 = consts[7], e2 = consts[8];
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) {
        const fp3 x = fp_mul(fp_load(a, j), k214);          // x 2^203
        fp3 r = x;                                          // the exponent's top bit (bit 180) is set
        for (int bit = 179; bit >= 0; --bit) {
            r = fp_mul(r, r);
            const uint64_t w = bit >= 128 ? e2 : (bit >= 64 ? e1 : e0);
            if ((w >> (bit & 63)) & 1) r = fp_mul(r, x);
        }
        fp_store(out, j, fp_mul(r, k192));
    }
}

// alt_bn128 Fr (bn254_dev.h): data live as x 2^256 and the device product divides by 2^261, so data x data = x y 2^251; there is no
// constant in a plain product to carry the missing 2^5, so one correcting product with the raw 2^266 is the price (consts[0]).
__global__ void __launch_bounds__(256) k_bn_mul(uint64_t *out, const uint64_t *a, const uint64_t *b, const uint64_t *consts, size_t n)
{
    const bn9 k266 = bnw_load(consts, 0);
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x)
        bnw_store_product(out, j, bn9_mul(bn9_mul(bnw_load(a, j), bnw_load(b, j)), k266));
}

// (a + 8r - b) times the table form of 1: the product is what makes the stored words canonical
__global__ void __launch_bounds__(256) k_bn_sub(uint64_t *out, const uint64_t *a, const uint64_t *b, size_t n)
{
    const bn9 one_t = bn9_const(BN9_C261);
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x)
        bnw_store_product(out, j, bn9_mul(bn9_add(bnw_load(a, j), bn9_negw(bnw_load(b, j))), one_t));
}

// Montgomery's trick over the BN_INV_BATCH positions a lane owns (j, j + 256, ...), all in registers: one Fermat inversion per batch.
// run_i = 2^261 prod_{l<=i} x_l 2^(-5 (i + 1)) (each stored factor carries 2^256 against the product's 2^-261); the inverse of the total,
// times 2^-5 once (consts[3], table form), makes before * inv = 2^261 / x_i at every step.  A multiple of r is stepped over as a stored 1
// and gives zero.  Reads of a position precede its write: out may alias a.
#define BN_INV_BATCH 4
__global__ void __launch_bounds__(256) k_bn_inv(uint64_t *out, const uint64_t *a, const uint64_t *consts, size_t n)
{
    const bn9 k256 = bnw_load(consts, 1), unscale_t = bnw_load(consts, 3), one_t = bn9_const(BN9_C261);
    for (size_t base = (size_t)blockIdx.x * (256 * BN_INV_BATCH); base < n; base += (size_t)gridDim.x * (256 * BN_INV_BATCH)) {
        for (unsigned lane = threadIdx.x; lane < 256; lane += blockDim.x) {
            bn9 x[BN_INV_BATCH], run[BN_INV_BATCH];
            bool zero[BN_INV_BATCH];
#pragma unroll
            for (int i = 0; i < BN_INV_BATCH; ++i) {
                const size_t j = base + lane + 256 * (size_t)i;
                x[i] = j < n ? bnw_load(a, j) : k256;
                zero[i] = bn9_is_zero_mod(x[i]);
                if (zero[i]) x[i] = k256;
                run[i] = bn9_mul(i ? run[i - 1] : one_t, x[i]);
            }
            bn9 inv = bn9_mul(bn9_fermat_inverse(run[BN_INV_BATCH - 1], consts + 8), unscale_t);
#pragma unroll
            for (int i = BN_INV_BATCH - 1; i >= 0; --i) {
                const size_t j = base + lane + 256 * (size_t)i;
                const bn9 q = bn9_mul(i ? run[i - 1] : one_t, inv);    // (1 / x_i) 2^261
                inv = bn9_mul(inv, x[i]);
                if (j < n) bnw_store_product(out, j, zero[i] ? bn9_zero() : bn9_mul(q, k256));
            }
        }
    }
}

// ---- random linear combination ---------------------------------------------------------------------------------------------
#define LINCOMB_MAX 16
struct LincombParams {
    const uint64_t *o[LINCOMB_MAX];
    const uint64_t *c;          // num coefficients (fp3: 2^203 form), then the constant term (libff's form) when has_constant
    uint64_t *out;
    int num, has_constant;
    size_t n;
};

__global__ void __launch_bounds__(256) k_lincomb_gf192(LincombParams p)
{
    const gf192 c0 = p.has_constant ? gf_load(p.c, p.num) : gf_zero();
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.n; j += (size_t)gridDim.x * blockDim.x) {
        gf192 acc = c0;
        for (int i = 0; i < p.num; ++i) gf_add_to(acc, gf_mul_uniform(gf_load(p.o[i], j), gf_load(p.c, i)));
        gf_store(p.out, j, acc);
    }
}

__global__ void __launch_bounds__(256) k_lincomb_fp3(LincombParams p)
{
    const fp3 c0 = p.has_constant ? fp_load(p.c, p.num) : fp_zero();
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.n; j += (size_t)gridDim.x * blockDim.x) {
        fp3 acc = c0;
        for (int g = 0; g < p.num; g += FP7W_MAX_TERMS) {    // up to 8 products per reduction (fp3_dev.h)
            fp7w w;
            fp7w_zero(w);
            const int e = g + FP7W_MAX_TERMS < p.num ? g + FP7W_MAX_TERMS : p.num;
            for (int i = g; i < e; ++i) fp_mac(w, fp_load(p.o[i], j), fp_load(p.c, i));
            acc = fp_add(acc, fp_redc(w));
        }
        fp_store(p.out, j, acc);
    }
}

// alt_bn128 Fr: four products per reduction; when a constant or a second group of four joins, the sum goes through one product with
// the table form of 1, which is what makes the stored words canonical (a single group of products with canonical coefficients is below 2r)
__global__ void __launch_bounds__(256) k_bn_lincomb(LincombParams p)
{
    const bn9 c0 = p.has_constant ? bnw_load(p.c, p.num) : bn9_zero(), one_t = bn9_const(BN9_C261);
    const bool direct = !p.has_constant && p.num <= 4;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.n; j += (size_t)gridDim.x * blockDim.x) {
        const bn9 acc = bn9_sum_products([&](size_t i) { return bnw_load(p.o[i], j); }, [&](size_t i) { return bnw_load(p.c, i); }, 0, (size_t)p.num);
        bnw_store_product(p.out, j, direct ? acc : bn9_mul(bn9_add(acc, c0), one_t));
    }
}

// ---- CSR sparse matrix x vector: one lane per row ----------------------------------------------------------------------------
struct SpmvParams {
    const uint64_t *row_ptr;    // rows + 1 offsets
    const uint32_t *col;
    const uint64_t *coeff, *vec;
    const uint64_t *scale;      // device: one element (fp3: r 2^214 raw, or 2^214 when there is no scale); gf192: nullable
    uint64_t *out;
    size_t rows;
    int accumulate;
};

__global__ void __launch_bounds__(256) k_spmv_gf192(SpmvParams p)
{
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < p.rows; r += (size_t)gridDim.x * blockDim.x) {
        gf192 acc = gf_zero();
        const uint64_t e = p.row_ptr[r + 1];
        for (uint64_t t = p.row_ptr[r]; t < e; ++t) gf_add_to(acc, gf_mul(gf_load(p.vec, p.col[t]), gf_load(p.coeff, t)));
        if (p.scale) acc = gf_mul(acc, gf_load(p.scale, 0));
        if (p.accumulate) gf_add_to(acc, gf_load(p.out, r));
        gf_store(p.out, r, acc);
    }
}

__global__ void __launch_bounds__(256) k_spmv_fp3(SpmvParams p)
{
    const fp3 k = fp_load(p.scale, 0);
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < p.rows; r += (size_t)gridDim.x * blockDim.x) {
        fp3 acc = fp_zero();                                  // sum of data x data products: scale 2^181
        const uint64_t e = p.row_ptr[r + 1];
        for (uint64_t t = p.row_ptr[r]; t < e; ++t) acc = fp_add(acc, fp_mul(fp_load(p.vec, p.col[t]), fp_load(p.coeff, t)));
        fp3 v = fp_mul(acc, k);
        if (p.accumulate) v = fp_add(v, fp_load(p.out, r));
        fp_store(p.out, r, v);
    }
}

// alt_bn128 Fr: the row sum at scale 2^251 (four products per reduction); scale (r 2^266 raw, or 2^266) restores libff's form in the
// same reduction that adds the previous content when accumulating
__global__ void __launch_bounds__(256) k_bn_spmv(SpmvParams p)
{
    const bn9 k = bnw_load(p.scale, 0), one_t = bn9_const(BN9_C261);
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < p.rows; r += (size_t)gridDim.x * blockDim.x) {
        const bn9 acc = bn9_sum_products([&](size_t t) { return bnw_load(p.vec, p.col[t]); }, [&](size_t t) { return bnw_load(p.coeff, t); },
                                         (size_t)p.row_ptr[r], (size_t)p.row_ptr[r + 1]);
        if (p.accumulate) {
            const bn9 a[2] = { acc, bnw_load(p.out, r) }, b[2] = { k, one_t };
            bnw_store_product(p.out, r, bn9_dot<2>(a, b));
        } else {
            bnw_store_product(p.out, r, bn9_mul(acc, k));
        }
    }
}

// ---- one factor (1 + u^(2^k)) of the power-series inverse ------------------------------------------------------------------
#define PDIV_MAX_TERMS 66
struct PolyDivParams {
    const uint64_t *src;
    uint64_t *dst;
    uint64_t consts[3 * PDIV_MAX_TERMS];     // nterms elements (fp3: 2^203 form; alt_bn128: four words each, 2^261 form), in the argument block: no upload launch per pass
    size_t off[PDIV_MAX_TERMS];
    size_t M;
    int nterms;
};

__global__ void __launch_bounds__(256) k_polydiv_pass_gf192(PolyDivParams p)
{
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.M; j += (size_t)gridDim.x * blockDim.x) {
        gf192 acc = gf_load(p.src, j);
        for (int t = 0; t < p.nterms; ++t) {
            const size_t s = j + p.off[t];
            if (s < p.M) gf_add_to(acc, gf_mul_uniform(gf_load(p.src, s), gf_load(p.consts, t)));
        }
        gf_store(p.dst, j, acc);
    }
}

__global__ void __launch_bounds__(256) k_polydiv_pass_fp3(PolyDivParams p)
{
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.M; j += (size_t)gridDim.x * blockDim.x) {
        fp3 acc = fp_load(p.src, j);
        for (int t = 0; t < p.nterms; ++t) {
            const size_t s = j + p.off[t];
            if (s < p.M) acc = fp_add(acc, fp_mul(fp_load(p.src, s), fp_load(p.consts, t)));
        }
        fp_store(p.dst, j, acc);
    }
}

// alt_bn128 Fr: src[j] 1 + sum_t src[j + off_t] c_t, each term in the reduction that also carries the running value; a position no
// term reaches is still multiplied by the table form of 1 (canonical words)
__global__ void __launch_bounds__(256) k_bn_polydiv_pass(PolyDivParams p)
{
    const bn9 one_t = bn9_const(BN9_C261);
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.M; j += (size_t)gridDim.x * blockDim.x) {
        bn9 acc = bnw_load(p.src, j);
        bool done = false;
        for (int t = 0; t < p.nterms; ++t) {
            const size_t s = j + p.off[t];
            if (s >= p.M) continue;
            const bn9 a[2] = { acc, bnw_load(p.src, s) }, b[2] = { one_t, bnw_load(p.consts, t) };
            acc = bn9_dot<2>(a, b);
            done = true;
        }
        bnw_store_product(p.dst, j, done ? acc : bn9_mul(acc, one_t));
    }
}

// The two prime fields' kernels of this file behind one host implementation (mul_field.h)
struct EoGf : Gf192Field {
    static constexpr auto lincomb = k_lincomb_gf192; static constexpr const char *lincomb_label = "k_lincomb_gf192";
    static constexpr auto spmv = k_spmv_gf192; static constexpr const char *spmv_label = "k_spmv_gf192";
};
struct EoFp : FpField {
    static constexpr auto lincomb = k_lincomb_fp3; static constexpr const char *lincomb_label = "k_lincomb_fp3";
    static constexpr auto spmv = k_spmv_fp3; static constexpr const char *spmv_label = "k_spmv_fp3";
    static constexpr auto mul = k_fp3_mul; static constexpr const char *mul_label = "k_fp3_mul";
    static constexpr auto sub = k_fp3_sub; static constexpr const char *sub_label = "k_fp3_sub";
    static constexpr auto inv = k_fp3_inv; static constexpr const char *inv_label = "k_fp3_inv";
    static constexpr auto polydiv_pass = k_polydiv_pass_fp3; static constexpr const char *polydiv_pass_label = "k_polydiv_pass_fp3";
    static int inv_grid(size_t n) { return eo_grid(n); }
};
struct EoBn : BnField {
    static constexpr auto lincomb = k_bn_lincomb; static constexpr const char *lincomb_label = "k_bn_lincomb";
    static constexpr auto spmv = k_bn_spmv; static constexpr const char *spmv_label = "k_bn_spmv";
    static constexpr auto mul = k_bn_mul; static constexpr const char *mul_label = "k_bn_mul";
    static constexpr auto sub = k_bn_sub; static constexpr const char *sub_label = "k_bn_sub";
    static constexpr auto inv = k_bn_inv; static constexpr const char *inv_label = "k_bn_inv";
    static constexpr auto polydiv_pass = k_bn_polydiv_pass; static constexpr const char *polydiv_pass_label = "k_bn_polydiv_pass";
    static int inv_grid(size_t n) { return eo_grid((n + BN_INV_BATCH - 1) / BN_INV_BATCH); }     // a lane owns a batch
};

// raw-word constants of the prime-field kernels, slots of F::WORDS: the device form of the stored 1 twice (2^214 / 2^266), the stored 1
// (2^192 / 2^256), p - 2, the table form of 1 / TABLE_FACTOR
template<class F>
static void fp_consts(uint64_t (&c)[4 * F::WORDS])
{
    typedef typename F::H H;
    const H k1 = H::one(), k2 = k1.table_form().table_form(), unscale_t = H::from_uint(F::TABLE_FACTOR).inverse().table_form();
    memcpy(c, k2.w, F::BYTES); memcpy(c + F::WORDS, k1.w, F::BYTES);
    for (int i = 0; i < F::WORDS; ++i) c[2 * F::WORDS + i] = H::P[i];
    c[2 * F::WORDS] -= 2;
    memcpy(c + 3 * F::WORDS, unscale_t.w, F::BYTES);
}

struct Term { size_t off; uint64_t c[4]; };

// runs the passes; `consts_of_pass(k)` yields the terms of the factor 1 + u^(2^k) (offsets already scaled).  Where a factor is 1 on the
// whole range the values are copied; with `canonical_copy` (alt_bn128 Fr, whose inputs may be raw words while every output is canonical)
// that copy is a pass with no terms, which stores each value times one.
template<typename PassTerms, typename Launch>
static int run_division(const uint64_t *d_high, size_t M, size_t min_offset, uint64_t *d_quotient, PassTerms terms_of_pass, Launch launch, size_t words = 3,
                        bool canonical_copy = false)
{
    const size_t elt = 8 * words;
    auto copy = [&](uint64_t *dst, const uint64_t *src) -> int {
        if (canonical_copy) {
            PolyDivParams p;
            memset(&p, 0, sizeof(p));
            p.src = src; p.dst = dst; p.M = M;      // elementwise: in place is fine
            return launch(p);
        }
        return src != dst ? iopx::copy_d2d(dst, src, M * elt) : IOPX_OK;
    };
    int passes = 0;
    for (size_t o = min_offset; o != 0 && o < M; o <<= 1) ++passes;         // offsets stay below 2 M <= 2^41: no overflow
    if (passes == 0) return copy(d_quotient, d_high);
    TmpBuf ping;
    int rc;
    if (passes > 1 && (rc = ping.alloc(M * elt)) != IOPX_OK) return rc;
    const uint64_t *src = d_high;
    for (int k = 0; k < passes; ++k) {
        // the last pass writes the quotient; before that alternate between the temporary and the quotient buffer
        uint64_t *dst = ((passes - 1 - k) & 1) ? ping.u64() : d_quotient;
        const std::vector<Term> terms = terms_of_pass(k);
        PolyDivParams p;
        memset(&p, 0, sizeof(p));
        for (const Term &t : terms) {
            if (t.off >= M) continue;
            memcpy(p.consts + words * p.nterms, t.c, elt);
            p.off[p.nterms++] = t.off;
        }
        if (p.nterms == 0) {        // nothing reaches back into the quotient: the factor is 1 on this range
            if ((rc = copy(dst, src)) != IOPX_OK) return rc;
            src = dst;
            continue;
        }
        p.src = src; p.dst = dst; p.M = M;
        if ((rc = launch(p)) != IOPX_OK) return rc;
        src = dst;
    }
    return IOPX_OK;
}

} // namespace iopx

using namespace iopx;

extern "C" {

int iopx_gf192_add_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (count == 0) return IOPX_OK;
    if (!d_a || !d_b || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    { ProfScope ps_("k_gf192_add"); hipLaunchKernelGGL(k_gf192_add, dim3(eo_grid(count)), dim3(256), 0, stream(), d_out, d_a, d_b, count); }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

int iopx_gf192_inv_dev(const uint64_t *d_a, uint64_t *d_out, size_t count)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (count == 0) return IOPX_OK;
    if (!d_a || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    { ProfScope ps_("k_gf192_inv"); hipLaunchKernelGGL(k_gf192_inv, dim3(eo_grid(count)), dim3(256), 0, stream(), d_out, d_a, count); }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

} // extern "C"

template<class F>
static int fp_elementwise(int op, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (count == 0) return IOPX_OK;
    if (!d_a || (op != 2 && !d_b) || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    uint64_t c[4 * F::WORDS];
    fp_consts<F>(c);
    TmpBuf dc;
    if ((rc = dc.alloc(sizeof(c))) != IOPX_OK) return rc;
    if ((rc = upload(dc.p, c, sizeof(c))) != IOPX_OK) return rc;
    if (op == 0) { ProfScope ps_(F::mul_label); hipLaunchKernelGGL(F::mul, dim3(eo_grid(count)), dim3(256), 0, stream(), d_out, d_a, d_b, (const uint64_t *)dc.u64(), count); }
    else if (op == 1) { ProfScope ps_(F::sub_label); hipLaunchKernelGGL(F::sub, dim3(eo_grid(count)), dim3(256), 0, stream(), d_out, d_a, d_b, count); }
    else { ProfScope ps_(F::inv_label); hipLaunchKernelGGL(F::inv, dim3(F::inv_grid(count)), dim3(256), 0, stream(), d_out, d_a, (const uint64_t *)dc.u64(), count); }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

extern "C" {

int iopx_fp3_mul_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count) { return fp_elementwise<EoFp>(0, d_a, d_b, d_out, count); }
int iopx_fp3_sub_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count) { return fp_elementwise<EoFp>(1, d_a, d_b, d_out, count); }
int iopx_fp3_inv_dev(const uint64_t *d_a, uint64_t *d_out, size_t count) { return fp_elementwise<EoFp>(2, d_a, nullptr, d_out, count); }
int iopx_bn128_mul_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count) { return fp_elementwise<EoBn>(0, d_a, d_b, d_out, count); }
int iopx_bn128_sub_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count) { return fp_elementwise<EoBn>(1, d_a, d_b, d_out, count); }
int iopx_bn128_inv_dev(const uint64_t *d_a, uint64_t *d_out, size_t count) { return fp_elementwise<EoBn>(2, d_a, nullptr, d_out, count); }

} // extern "C"

template<class F>
static int lincomb_common(const void *const *d_oracles, size_t num, const uint64_t *coeffs, const uint64_t *constant, size_t n, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_oracles || !coeffs || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (num == 0 || num > LINCOMB_MAX) return fail(IOPX_ERR_INVALID_ARGUMENT, "Random Linear Combination Oracle: Expected same number of evaluations as in registration.");
    std::vector<uint64_t> hc(F::WORDS * num);
    multiplier_words<F>(coeffs, num, hc.data());
    if (constant) hc.insert(hc.end(), constant, constant + F::WORDS);
    TmpBuf dc;
    if ((rc = dc.alloc(hc.size() * 8)) != IOPX_OK) return rc;
    if ((rc = upload(dc.p, hc.data(), hc.size() * 8)) != IOPX_OK) return rc;
    LincombParams p;
    memset(&p, 0, sizeof(p));
    for (size_t i = 0; i < num; ++i) { if (!d_oracles[i]) return fail(IOPX_ERR_INVALID_ARGUMENT, "null oracle"); p.o[i] = (const uint64_t *)d_oracles[i]; }
    p.c = dc.u64(); p.out = d_out; p.num = (int)num; p.n = n; p.has_constant = constant ? 1 : 0;
    { ProfScope ps_(F::lincomb_label, (num + 1) * n * F::BYTES); hipLaunchKernelGGL(F::lincomb, dim3(eo_grid(n)), dim3(256), 0, stream(), p); }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int spmv_common(const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_coeff, size_t rows, const uint64_t *d_vec,
                       const uint64_t *scale, int accumulate, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (rows == 0) return IOPX_OK;
    if (!d_row_ptr || !d_col || !d_coeff || !d_vec || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    SpmvParams p;
    p.row_ptr = d_row_ptr; p.col = d_col; p.coeff = d_coeff; p.vec = d_vec; p.out = d_out; p.rows = rows; p.accumulate = accumulate; p.scale = nullptr;
    TmpBuf ds;
    uint64_t k[F::WORDS];
    bool have = scale != nullptr;
    if constexpr (F::PRIME) {       // always a constant: it also rescales the data x data products (r 2^214 / r 2^266 raw)
        const typename F::H t = (scale ? F::H::from_words(scale) : F::H::one()).table_form().table_form();
        memcpy(k, t.w, F::BYTES);
        have = true;
    } else if (scale) {
        memcpy(k, scale, F::BYTES);
    }
    if (have) {
        if ((rc = ds.alloc(F::BYTES)) != IOPX_OK) return rc;
        if ((rc = upload(ds.p, k, F::BYTES)) != IOPX_OK) return rc;
        p.scale = ds.u64();
    }
    { ProfScope ps_(F::spmv_label); hipLaunchKernelGGL(F::spmv, dim3(eo_grid(rows)), dim3(256), 0, stream(), p); }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

extern "C" {

int iopx_lincomb_gf192_dev(const void *const *d_oracles, size_t num_oracles, const uint64_t *coefficients, size_t n, uint64_t *d_out)
{
    return lincomb_common<EoGf>(d_oracles, num_oracles, coefficients, nullptr, n, d_out);
}
int iopx_lincomb_fp3_dev(const void *const *d_oracles, size_t num_oracles, const uint64_t *coefficients, size_t n, uint64_t *d_out)
{
    return lincomb_common<EoFp>(d_oracles, num_oracles, coefficients, nullptr, n, d_out);
}
int iopx_lincomb_bn128_dev(const void *const *d_oracles, size_t num_oracles, const uint64_t *coefficients, size_t n, uint64_t *d_out)
{
    return lincomb_common<EoBn>(d_oracles, num_oracles, coefficients, nullptr, n, d_out);
}
// sum_i c_i o_i + constant: single_matrix_denominator::evaluated_contents (libiop/protocols/encoded/lincheck/holographic_lincheck_aux.tcc:117-143)
int iopx_lincomb_affine_gf192_dev(const void *const *d_oracles, size_t num_oracles, const uint64_t *coefficients, const uint64_t *constant, size_t n,
                                  uint64_t *d_out)
{
    if (!constant) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    return lincomb_common<EoGf>(d_oracles, num_oracles, coefficients, constant, n, d_out);
}
int iopx_lincomb_affine_fp3_dev(const void *const *d_oracles, size_t num_oracles, const uint64_t *coefficients, const uint64_t *constant, size_t n,
                                uint64_t *d_out)
{
    if (!constant) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    return lincomb_common<EoFp>(d_oracles, num_oracles, coefficients, constant, n, d_out);
}
int iopx_lincomb_affine_bn128_dev(const void *const *d_oracles, size_t num_oracles, const uint64_t *coefficients, const uint64_t *constant, size_t n,
                                  uint64_t *d_out)
{
    if (!constant) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    return lincomb_common<EoBn>(d_oracles, num_oracles, coefficients, constant, n, d_out);
}

int iopx_spmv_gf192_dev(const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_coeff, size_t rows, const uint64_t *d_vec,
                        const uint64_t *scale, int accumulate, uint64_t *d_out)
{
    return spmv_common<EoGf>(d_row_ptr, d_col, d_coeff, rows, d_vec, scale, accumulate, d_out);
}
int iopx_spmv_fp3_dev(const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_coeff, size_t rows, const uint64_t *d_vec,
                      const uint64_t *scale, int accumulate, uint64_t *d_out)
{
    return spmv_common<EoFp>(d_row_ptr, d_col, d_coeff, rows, d_vec, scale, accumulate, d_out);
}
int iopx_spmv_bn128_dev(const uint64_t *d_row_ptr, const uint32_t *d_col, const uint64_t *d_coeff, size_t rows, const uint64_t *d_vec,
                        const uint64_t *scale, int accumulate, uint64_t *d_out)
{
    return spmv_common<EoBn>(d_row_ptr, d_col, d_coeff, rows, d_vec, scale, accumulate, d_out);
}

int iopx_poly_div_vanishing_gf192_dev(const uint64_t *d_poly, size_t n_coeffs, const uint64_t *basis, size_t dim, const uint64_t *shift,
                                      uint64_t *d_quotient)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_poly || (dim > 0 && !basis) || !shift || !d_quotient) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (dim > 62) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension too large");
    const size_t N = (size_t)1 << dim;
    if (n_coeffs <= N) return IOPX_OK;                       // empty quotient (linearized_polynomial.tcc:247-255)
    const size_t M = n_coeffs - N;
    // Z = sum_{i <= dim} lin[i] X^(2^i) + lin(shift): the subspace polynomial built factor by factor (vanishing_polynomial.tcc:373-395)
    std::vector<hgf192> lin(1, hgf192::one());
    auto eval = [&](const hgf192 &x) { hgf192 r = hgf192::zero(), xp = x; for (size_t i = 0; i < lin.size(); ++i) { r += lin[i] * xp; xp = xp.squared(); } return r; };
    for (size_t k = 0; k < dim; ++k) {
        const hgf192 zb = eval(hgf192::from_words(basis + 3 * k));
        std::vector<hgf192> nxt(lin.size() + 1, hgf192::zero());
        for (size_t i = 0; i < lin.size(); ++i) { nxt[i + 1] += lin[i].squared(); nxt[i] += lin[i] * zb; }
        lin.swap(nxt);
    }
    if (!(lin[dim] == hgf192::one())) return fail(IOPX_ERR_LOGIC, "vanishing polynomial is not monic");
    const hgf192 c_const = eval(hgf192::from_words(shift));
    std::vector<hgf192> cur;                                 // c_i^(2^k), squared once per pass
    std::vector<size_t> base_off;
    for (size_t i = 0; i < dim; ++i) if (!lin[i].is_zero()) { cur.push_back(lin[i]); base_off.push_back(N - ((size_t)1 << i)); }
    if (!c_const.is_zero()) { cur.push_back(c_const); base_off.push_back(N); }
    if (cur.size() > PDIV_MAX_TERMS) return fail(IOPX_ERR_INVALID_ARGUMENT, "too many terms");
    size_t min_off = 0;
    for (size_t o : base_off) if (min_off == 0 || o < min_off) min_off = o;
    int done = 0;
    auto terms_of_pass = [&](int k) {
        while (done < k) { for (hgf192 &c : cur) c = c.squared(); ++done; }
        std::vector<Term> t;
        for (size_t i = 0; i < cur.size(); ++i) {
            Term x;
            x.off = base_off[i] << k;
            memcpy(x.c, cur[i].w, 24);
            t.push_back(x);
        }
        return t;
    };
    auto launch = [&](const PolyDivParams &p) -> int {
        { ProfScope ps_("k_polydiv_pass_gf192", 2 * (size_t)p.M * 24); hipLaunchKernelGGL(k_polydiv_pass_gf192, dim3(eo_grid(p.M)), dim3(256), 0, stream(), p); }
        IOPX_HIP(hipGetLastError());
        return IOPX_OK;
    };
    if (cur.empty()) min_off = 0;
    return run_division(d_poly + 3 * N, M, min_off, d_quotient, terms_of_pass, launch);
}

} // extern "C"

template<class F>
static int poly_div_vanishing_mul(const uint64_t *d_poly, size_t n_coeffs, size_t log_order, const uint64_t *shift, uint64_t *d_quotient)
{
    typedef typename F::H H;
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_poly || !shift || !d_quotient) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (log_order > (size_t)F::TWO_ADICITY) return fail(IOPX_ERR_INVALID_ARGUMENT, "log_order %zu exceeds the 2-adicity of %s", log_order, F::TWO_ADICITY == 31 ? "the field" : F::NAME);
    const size_t N = (size_t)1 << log_order;
    if (n_coeffs <= N) return IOPX_OK;
    const size_t M = n_coeffs - N;
    // Z = X^N - c, c = shift^N (vanishing_polynomial.tcc:14-25): Q_j = P_{j+N} + c Q_{j+N}
    H cur = H::from_words(shift).pow((uint64_t)N);
    int done = 0;
    auto terms_of_pass = [&](int k) {
        while (done < k) { cur = cur.squared(); ++done; }
        Term x;
        x.off = N << k;
        const H t = cur.table_form();
        memcpy(x.c, t.w, F::BYTES);
        return std::vector<Term>(1, x);
    };
    auto launch = [&](const PolyDivParams &p) -> int {
        { ProfScope ps_(F::polydiv_pass_label); hipLaunchKernelGGL(F::polydiv_pass, dim3(eo_grid(p.M)), dim3(256), 0, stream(), p); }
        IOPX_HIP(hipGetLastError());
        return IOPX_OK;
    };
    return run_division(d_poly + F::WORDS * N, M, N, d_quotient, terms_of_pass, launch, F::WORDS, F::RAW_INPUTS);
}

extern "C" {

int iopx_poly_div_vanishing_fp3_dev(const uint64_t *d_poly, size_t n_coeffs, size_t log_order, const uint64_t *shift, uint64_t *d_quotient)
{ return poly_div_vanishing_mul<EoFp>(d_poly, n_coeffs, log_order, shift, d_quotient); }
int iopx_poly_div_vanishing_bn128_dev(const uint64_t *d_poly, size_t n_coeffs, size_t log_order, const uint64_t *shift, uint64_t *d_quotient)
{ return poly_div_vanishing_mul<EoBn>(d_poly, n_coeffs, log_order, shift, d_quotient); }

} // extern "C"
