// Multiplicative-coset FFT / IFFT, FRI fold and LDT combination over alt_bn128 Fr (254 bits, 2-adicity 28) for gfx950.
//
// The alt_bn128 arm of fft_mul.hip (edwards_Fr) and of k_ldt_combine_fp (ldt_reducer.hip), with the same structure and
// semantics; it replaces, for multiplicative domains (reference paths relative to the libiop tree):
//   multiplicative_FFT_degree_aware      libiop/algebra/fft.tcc:236-317   (a[i] = P(shift * g^i), natural order)
//   multiplicative_IFFT_internal         libiop/algebra/fft.tcc:343-361   -> libfqfft basic_radix2_domain::iFFT / icosetFFT
//   IFFT_of_known_degree (mult.)         libiop/algebra/fft.tcc:435-456   (strided gather + IFFT on the sub-coset)
//   multiplicative_evaluate_next_f_i_... libiop/protocols/ldt/fri/fri_aux.tcc:106-249
//   combined_LDT_virtual_oracle::evaluated_contents, multiplicative arm, ldt_reducer_aux.tcc:104-128
//
// Elements are libff Fp_model<4> Montgomery words (x * 2^256 mod r, four little-endian uint64, canonical at the boundary).
// Products run on bn254_dev.h's nine 29-bit limbs, whose Montgomery product divides by 2^261: data stay in the library's
// x * 2^256 form throughout and every multiplier (twiddles, shift powers, n^-1, 1/2, fold and LDT constants) is kept in
// "table form" t * 2^261 (hbn::table_form), so x 2^256 * t 2^261 / 2^261 = x t 2^256 and no conversion is ever needed.
// Between operations a value is any representative below 2^256 with normalised limbs ("weak"); sums and differences are
// brought back below 2^256 by bn9_reduce, products of weak values are below 2r.  Kernels store canonical words.
#include <hip/hip_runtime.h>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include "bn254_dev.h"
#include "bn254_host.h"
#include "runtime.h"

namespace iopx {

// tile geometry of k_bn_mfft_pass: 2048-element tiles (64 KiB of LDS at 32 bytes an element), 16 columns in the strided passes
static const int BF_TILE_BITS = 11;
static const int BF_COLS = 4;

// 2^261 mod r, plain limbs: a product with it maps a weak x * 2^256 value to a representative below 2r of the same residue
__device__ static const uint32_t BN9_C261[9] = { 0x0fffff57u, 0x1ea70ab4u, 0x052c068bu, 0x17504f49u, 0x0aa8075bu, 0x1d4240ceu, 0x11d54c07u, 0x052ac7a8u, 0x000dc836u };
// 8r with a 2^29 borrowed into limbs 0..7 from the limb above: limbs 0..7 in [2^29, 2^30), limb 8 above 2^24, so that
// 8r - b is limb-wise non-negative for any weak b (normalised limbs, value below 2^256)
__device__ static const uint32_t BN9_8R[9] = { 0x20000008u, 0x387d64fbu, 0x32e12286u, 0x3e84879au, 0x2c2e9418u, 0x36da0604u, 0x25370a07u, 0x32e1319fu, 0x01832272u };

__device__ __forceinline__ bn9 bnw_load(const uint64_t *__restrict__ p, size_t idx) { return bn9_unpack(p + 4 * idx); }

// weak value (normalised limbs, below 2^256) -> four words, no reduction
__device__ __forceinline__ void bnw_pack(uint64_t *q, const bn9 &y)
{
    uint32_t w[8];
    uint64_t acc = 0;
    int bits = 0, wi = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        acc |= (uint64_t)y.l[i] << bits;
        bits += 29;
        if (bits >= 32 && wi < 8) { w[wi++] = (uint32_t)acc; acc >>= 32; bits -= 32; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
}

// weak -> canonical words
__device__ __forceinline__ void bnw_store(uint64_t *p, size_t idx, const bn9 &v) { bn9_store_canonical(p + 4 * idx, bn9_mul(v, bn9_const(BN9_C261))); }
// a product (below 2r) -> canonical words
__device__ __forceinline__ void bnw_store_product(uint64_t *p, size_t idx, const bn9 &v) { bn9_store_canonical(p + 4 * idx, v); }

__device__ __forceinline__ bn9 bnw_add(const bn9 &a, const bn9 &b) { return bn9_reduce(bn9_add(a, b)); }

__device__ __forceinline__ bn9 bnw_sub(const bn9 &a, const bn9 &b)
{
    bn9 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = a.l[i] + BN9_8R[i] - b.l[i];
    return bn9_reduce(r);
}

// (a, b) <- (a + w b, a - w b)   (fft.tcc:303-309); w in table form
__device__ __forceinline__ void bnw_bfly(bn9 &a, bn9 &b, const bn9 &w)
{
    const bn9 t = bn9_mul(b, w);
    b = bnw_sub(a, t);
    a = bnw_add(a, t);
}

__device__ __forceinline__ bn9 blds_get(const uint64_t *s, int E, int li)
{
    const uint64_t q[4] = { s[li], s[E + li], s[2 * E + li], s[3 * E + li] };
    return bn9_unpack(q);
}

__device__ __forceinline__ void blds_put(uint64_t *s, int E, int li, const bn9 &v)
{
    uint64_t q[4];
    bnw_pack(q, v);
    s[li] = q[0]; s[E + li] = q[1]; s[2 * E + li] = q[2]; s[3 * E + li] = q[3];
}

// out[q] = init * prod_{k : bit k of q} sq[k]   (sq[k] = base^(2^k)), q < count; all in table form
__global__ void k_bn_pow_direct(uint64_t *out, const uint64_t *sq, const uint64_t *init, int nbits, size_t count)
{
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < count; q += (size_t)gridDim.x * blockDim.x) {
        bn9 acc = bnw_load(init, 0);
        for (int k = 0; k < nbits; ++k) {
            if ((q >> k) & 1) acc = bn9_mul(acc, bnw_load(sq, k));
        }
        bnw_store_product(out, q, acc);        // init is canonical; products are below 2r
    }
}

// out[q] = out[q & 255] * hi[q >> 8]  for 256 <= q < count
__global__ void k_bn_pow_expand(uint64_t *out, const uint64_t *hi, size_t count)
{
    for (size_t q = 256 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < count; q += (size_t)gridDim.x * blockDim.x) {
        bnw_store_product(out, q, bn9_mul(bnw_load(out, q & 255), bnw_load(hi, q >> 8)));
    }
}

// cache level with m = 2^b entries at offset m - 1: entry j = top[j << (logn - 1 - b)]   (subgroup.tcc:117-144)
__global__ void k_bn_cache_level(uint64_t *cache, int logn, int b)
{
    const size_t m = (size_t)1 << b;
    const uint64_t *top = cache + 4 * ((((size_t)1) << (logn - 1)) - 1);
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (size_t)gridDim.x * blockDim.x) {
        const uint64_t *s = top + 4 * (j << (logn - 1 - b));
        uint64_t *d = cache + 4 * (m - 1 + j);
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
    }
}

// dst[k] = src[k] * hi[k >> 12] * lo[k & 4095]      (coset pre-scaling a[k] *= shift^k, fft.tcc:246-249)
__global__ void k_bn_scale_pow(uint64_t *dst, const uint64_t *src, const uint64_t *hi, const uint64_t *lo, size_t count)
{
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (size_t)gridDim.x * blockDim.x) {
        bnw_store_product(dst, k, bn9_mul(bnw_load(src, k), bn9_mul(bnw_load(hi, k >> 12), bnw_load(lo, k & 4095))));
    }
}

__global__ void k_bn_gather_stride(uint64_t *dst, const uint64_t *src, size_t stride, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < 4 * count; i += (size_t)gridDim.x * blockDim.x) {
        dst[i] = src[4 * ((i / 4) * stride) + (i % 4)];
    }
}

struct BfParams {
    const uint64_t *src;    // first pass: coefficient / evaluation array of n_src elements (gathered bit-reversed)
    uint64_t *dst;
    const uint64_t *cache;  // n - 1 twiddles, level b at offset 2^b - 1
    const uint64_t *sc_hi, *sc_lo;  // last pass: out[i] *= sc_hi[i >> 12] * sc_lo[i & 4095]   (null: no scaling)
    size_t n_src;
    int logn, logrho;       // index bits [logrho, logn) are active; the low logrho bits replicate
    int gather;
    int c, h, A;            // tile: columns on bits [0,c), rows on bits [h, h+A)
    int b_lo, b_hi;         // butterfly bits of this pass (ascending)
    int scale;              // 0 none, 1 sc_hi[0] only (n^-1), 2 two-level table
    int final;              // last pass of a transform: store canonical values (earlier passes store weak ones)
};

// R levels starting at global index bit b on 2^R elements per lane (local indices i0 | k << bl), as mfft_step in fft_mul.hip
template<int R>
__device__ __forceinline__ void bn_mfft_step(uint64_t *s, int E, const BfParams &p, size_t base, int cmask, int b, int tid, int nt)
{
    const int bl = b - p.h + p.c;                           // tile-local bit of level b
    for (int grp = tid; grp < (E >> R); grp += nt) {
        const int low = grp & ((1 << bl) - 1), high = grp >> bl;
        const int i0 = (high << (bl + R)) | low;
        const size_t gi0 = base | ((size_t)(i0 >> p.c) << p.h) | (size_t)(i0 & cmask);
        const size_t lowidx = gi0 & ((((size_t)1) << b) - 1);
        bn9 v[1 << R];
#pragma unroll
        for (int k = 0; k < (1 << R); ++k) v[k] = blds_get(s, E, i0 | (k << bl));
#pragma unroll
        for (int lev = 0; lev < R; ++lev) {
            const uint64_t *lvl = p.cache + 4 * ((((size_t)1) << (b + lev)) - 1);
#pragma unroll
            for (int q = 0; q < (1 << lev); ++q) {
                const bn9 w = bnw_load(lvl, lowidx + ((size_t)q << b));
#pragma unroll
                for (int k = 0; k < (1 << R); ++k) {
                    if ((k & ((1 << lev) - 1)) == q && !((k >> lev) & 1)) bnw_bfly(v[k], v[k | (1 << lev)], w);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < (1 << R); ++k) blds_put(s, E, i0 | (k << bl), v[k]);
    }
}

__global__ void __launch_bounds__(256) k_bn_mfft_pass(BfParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t iopx_smem[];
    uint64_t *s = iopx_smem;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int E = 1 << (p.c + p.A);
    const int midbits = p.h - p.c;
    const size_t o = blockIdx.x;
    const size_t mid = o & (((size_t)1 << midbits) - 1), hi = o >> midbits;
    const size_t base = (hi << (p.h + p.A)) | (mid << p.c);
    const int cmask = (1 << p.c) - 1;
    const int logd = p.logn - p.logrho;

    for (int li = tid; li < E; li += nt) {
        const size_t gi = base | ((size_t)(li >> p.c) << p.h) | (size_t)(li & cmask);
        const uint64_t *q = nullptr;
        if (p.gather) {
            const size_t t = gi >> p.logrho;
            const size_t k = logd == 0 ? 0 : (size_t)(__brevll((unsigned long long)t) >> (64 - logd));
            if (k < p.n_src) q = p.src + 4 * k;
        } else {
            q = p.src + 4 * gi;
        }
        s[li] = q ? q[0] : 0; s[E + li] = q ? q[1] : 0; s[2 * E + li] = q ? q[2] : 0; s[3 * E + li] = q ? q[3] : 0;
    }
    __syncthreads();

    // radix-8 / 4 / 2 steps: one LDS round trip and one barrier per three levels
    int b = p.b_lo;
    for (; b + 2 <= p.b_hi; b += 3) { bn_mfft_step<3>(s, E, p, base, cmask, b, tid, nt); __syncthreads(); }
    if (b + 1 <= p.b_hi) { bn_mfft_step<2>(s, E, p, base, cmask, b, tid, nt); __syncthreads(); b += 2; }
    if (b <= p.b_hi) { bn_mfft_step<1>(s, E, p, base, cmask, b, tid, nt); __syncthreads(); }

    for (int li = tid; li < E; li += nt) {
        const size_t gi = base | ((size_t)(li >> p.c) << p.h) | (size_t)(li & cmask);
        const bn9 v = blds_get(s, E, li);
        if (p.scale == 1) bnw_store_product(p.dst, gi, bn9_mul(v, bnw_load(p.sc_hi, 0)));
        else if (p.scale == 2) bnw_store_product(p.dst, gi, bn9_mul(v, bn9_mul(bnw_load(p.sc_hi, gi >> 12), bnw_load(p.sc_lo, gi & 4095))));
        else if (p.final) bnw_store(p.dst, gi, v);
        else { uint64_t *d = p.dst + 4 * gi; d[0] = s[li]; d[1] = s[E + li]; d[2] = s[2 * E + li]; d[3] = s[3 * E + li]; }
    }
}

struct BfoldParams {
    const uint64_t *src;
    uint64_t *dst;
    const uint64_t *ginv;   // g^-j for j < n0/2 (top level of the inverse cache), table form
    const uint64_t *consts; // per level: [2e] = x / shift, [2e + 1] = 1/2, table form
    size_t half;            // outputs = pairs (j, j + half)
    int stride_log;         // ginv index = j << stride_log
};

// g[j] = ((a + b) + (a - b) * (x / shift) * g^-j) / 2
__global__ void k_bn_fri_fold2(BfoldParams p)
{
    const bn9 xs = bnw_load(p.consts, 0), inv2 = bnw_load(p.consts, 1);
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.half; j += (size_t)gridDim.x * blockDim.x) {
        const bn9 a = bnw_load(p.src, j), b = bnw_load(p.src, j + p.half);
        const bn9 c = bn9_mul(xs, bnw_load(p.ginv, j << p.stride_log));
        const bn9 r = bnw_add(bnw_add(a, b), bn9_mul(bnw_sub(a, b), c));
        bnw_store_product(p.dst, j, bn9_mul(r, inv2));
    }
}

// one kernel per FRI round for cosets of 2^ETA (k_fri_fold_fused_mul in fft_mul.hip): a lane loads f[j + t q], t < 2^ETA,
// folds ETA times in registers and writes one element
template<int ETA>
__global__ void __launch_bounds__(256) k_bn_fri_fold_fused(BfoldParams p)
{
    const size_t q = p.half;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < q; j += (size_t)gridDim.x * blockDim.x) {
        bn9 v[1 << ETA];
#pragma unroll
        for (int t = 0; t < (1 << ETA); ++t) v[t] = bnw_load(p.src, j + (size_t)t * q);
#pragma unroll
        for (int e = 0; e < ETA; ++e) {
            const bn9 xs = bnw_load(p.consts, 2 * e), inv2 = bnw_load(p.consts, 2 * e + 1);
            const int pairs = 1 << (ETA - 1 - e);
#pragma unroll
            for (int t = 0; t < pairs; ++t) {
                const size_t u = j + (size_t)t * q;                             // index in the level-e array
                const bn9 c = bn9_mul(xs, bnw_load(p.ginv, u << e));
                const bn9 a = v[t], b = v[t + pairs];
                v[t] = bn9_mul(bnw_add(bnw_add(a, b), bn9_mul(bnw_sub(a, b), c)), inv2);
            }
        }
        bnw_store_product(p.dst, j, v[0]);
    }
}

struct BldtParams {
    const uint64_t *const *oracles; // device array of num_oracles device pointers
    const uint64_t *const *hi;      // per oracle: hi table (nullptr = maximal)
    const uint64_t *const *lo;
    uint64_t *out;
    const uint64_t *coef;           // per oracle: c[k], table form
    size_t n;
    int num_oracles;
};

// out[j] = sum_o (c_o + c'_o shift^e_o (g^e_o)^j) f_o[j]   (ldt_reducer_aux.tcc:104-128)
__global__ void __launch_bounds__(256) k_bn_ldt_combine(BldtParams p)
{
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.n; j += (size_t)gridDim.x * blockDim.x) {
        bn9 acc = bn9_zero();
        for (int o = 0; o < p.num_oracles; ++o) {
            bn9 c = bnw_load(p.coef, o);
            const uint64_t *hi = p.hi[o];
            if (hi) c = bnw_add(c, bn9_mul(bnw_load(hi, j >> 12), bnw_load(p.lo[o], j & 4095)));
            acc = bnw_add(acc, bn9_mul(c, bnw_load(p.oracles[o], j)));
        }
        bnw_store(p.out, j, acc);
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static const size_t BN_BYTES = 32;
static const int BN_TWO_ADICITY = 28;

struct BnPlan {
    int logn = 0;
    hbn g, ginv;
    DevBuf cache_fwd, cache_inv;        // n - 1 twiddles each (table form), built on first use
    bool have_fwd = false, have_inv = false;
};

static std::mutex g_bnplan_mu;
static std::map<std::vector<uint64_t>, std::unique_ptr<BnPlan>> g_bnplans;

void clear_bn128_plans()
{
    std::lock_guard<std::mutex> lk(g_bnplan_mu);
    g_bnplans.clear();
}

static int bgrid(size_t work, int threads)
{
    size_t g = (work + threads - 1) / threads;
    if (g < 1) g = 1;
    if (g > 8192) g = 8192;
    return (int)g;
}

// out[q] = init * base^q for q < 2^nb, table form (base and init are ordinary elements)
static int bn_build_pow(uint64_t *out, const hbn &base, const hbn &init, int nb)
{
    std::vector<uint64_t> sq;
    hbn x = base;
    for (int k = 0; k < nb; ++k) { const hbn t = x.table_form(); sq.insert(sq.end(), t.w, t.w + 4); x = x.squared(); }
    const hbn init_t = init.table_form();
    const size_t init_at = sq.size();
    sq.insert(sq.end(), init_t.w, init_t.w + 4);
    TmpBuf dsq;
    int rc;
    if ((rc = dsq.alloc(sq.size() * 8)) != IOPX_OK) return rc;
    if ((rc = upload(dsq.p, sq.data(), sq.size() * 8)) != IOPX_OK) return rc;
    const uint64_t *dinit = dsq.u64() + init_at;
    const size_t count = (size_t)1 << nb;
    if (nb <= 14) {
        { ProfScope ps_("k_bn_pow_direct"); hipLaunchKernelGGL(k_bn_pow_direct, dim3(bgrid(count, 256)), dim3(256), 0, stream(), out, (const uint64_t *)dsq.u64(), dinit, nb, count); }
    } else {
        // out[0..256) = init * base^q ; hi[r] = (base^256)^r ; out[q] = out[q & 255] * hi[q >> 8]
        TmpBuf hi;
        if ((rc = hi.alloc((((size_t)1) << (nb - 8)) * BN_BYTES)) != IOPX_OK) return rc;
        hbn b256 = base;
        for (int k = 0; k < 8; ++k) b256 = b256.squared();
        if ((rc = bn_build_pow(hi.u64(), b256, hbn::one(), nb - 8)) != IOPX_OK) return rc;
        { ProfScope ps_("k_bn_pow_direct"); hipLaunchKernelGGL(k_bn_pow_direct, dim3(1), dim3(256), 0, stream(), out, (const uint64_t *)dsq.u64(), dinit, 8, (size_t)256); }
        { ProfScope ps_("k_bn_pow_expand"); hipLaunchKernelGGL(k_bn_pow_expand, dim3(bgrid(count - 256, 256)), dim3(256), 0, stream(), out, (const uint64_t *)hi.u64(), count); }
    }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;         // temporaries are released in stream order
}

// two-level power tables: hi[q] = init * base^(4096 q) (q < 2^max(logc-12,0)), lo[r] = base^r (r < min(2^logc, 4096))
static int bn_build_two_level(const hbn &base, const hbn &init, int logc, TmpBuf &hi, TmpBuf &lo)
{
    const int lo_bits = logc < 12 ? logc : 12, hi_bits = logc > 12 ? logc - 12 : 0;
    int rc;
    if ((rc = lo.alloc((((size_t)1) << lo_bits) * BN_BYTES)) != IOPX_OK) return rc;
    if ((rc = bn_build_pow(lo.u64(), base, hbn::one(), lo_bits)) != IOPX_OK) return rc;
    hbn b4096 = base;
    for (int k = 0; k < 12; ++k) b4096 = b4096.squared();
    if ((rc = hi.alloc((((size_t)1) << hi_bits) * BN_BYTES)) != IOPX_OK) return rc;
    return bn_build_pow(hi.u64(), b4096, init, hi_bits);
}

static int bn_build_cache(BnPlan &pl, bool inverse)
{
    ColdScope cold_("alt_bn128 multiplicative FFT twiddle cache");
    const int logn = pl.logn;
    DevBuf &buf = inverse ? pl.cache_inv : pl.cache_fwd;
    const size_t n = (size_t)1 << logn;
    int rc = buf.alloc((n > 1 ? n - 1 : 1) * BN_BYTES);
    if (rc != IOPX_OK) return rc;
    if (logn >= 1) {
        uint64_t *top = buf.u64() + 4 * ((n >> 1) - 1);
        if ((rc = bn_build_pow(top, inverse ? pl.ginv : pl.g, hbn::one(), logn - 1)) != IOPX_OK) return rc;
        for (int b = 0; b < logn - 1; ++b) {
            { ProfScope ps_("k_bn_cache_level"); hipLaunchKernelGGL(k_bn_cache_level, dim3(bgrid((size_t)1 << b, 256)), dim3(256), 0, stream(), buf.u64(), logn, b); }
        }
        IOPX_HIP(hipStreamSynchronize(stream()));
    }
    (inverse ? pl.have_inv : pl.have_fwd) = true;
    return IOPX_OK;
}

static int bn_get_plan(int logn, const uint64_t *gen, BnPlan **out)
{
    std::vector<uint64_t> key(gen, gen + 4);
    key.push_back((uint64_t)logn);
    std::lock_guard<std::mutex> lk(g_bnplan_mu);
    auto it = g_bnplans.find(key);
    if (it != g_bnplans.end()) { *out = it->second.get(); return IOPX_OK; }
    std::unique_ptr<BnPlan> pl(new BnPlan());
    pl->logn = logn;
    pl->g = hbn::from_words(gen);
    if (pl->g.is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "alt_bn128 multiplicative FFT: zero generator");
    if (!(pl->g.pow((uint64_t)1 << logn) == hbn::one()) || (logn > 0 && pl->g.pow((uint64_t)1 << (logn - 1)) == hbn::one()))
        return fail(IOPX_ERR_INVALID_ARGUMENT, "alt_bn128 multiplicative FFT: generator does not have order 2^%d", logn);
    pl->ginv = pl->g.inverse();
    *out = pl.get();
    g_bnplans[key] = std::move(pl);
    return IOPX_OK;
}

// the radix-2 levels on index bits [logrho, logn) (the first pass gathers src bit-reversed), natural-order dst
static int bn_run_mfft(const uint64_t *cache, const uint64_t *src, size_t n_src, uint64_t *dst, int logn, int logrho,
                       int scale, const uint64_t *sc_hi, const uint64_t *sc_lo)
{
    struct Pass { int c, h, A, b_lo, b_hi; };
    std::vector<Pass> passes;
    int b = logrho;
    if (logn <= BF_TILE_BITS) {
        passes.push_back({0, 0, logn, b, logn - 1});
        b = logn;
    } else if (logrho < BF_TILE_BITS) {
        passes.push_back({0, 0, BF_TILE_BITS, b, BF_TILE_BITS - 1});
        b = BF_TILE_BITS;
    }
    while (b < logn) {
        int A = BF_TILE_BITS - BF_COLS;
        if (b + A > logn) A = logn - b;
        int c = BF_TILE_BITS - A;
        if (c > b) c = b;
        passes.push_back({c, b, A, b, b + A - 1});
        b += A;
    }
    if (passes.empty()) passes.push_back({0, 0, logn < BF_TILE_BITS ? logn : BF_TILE_BITS, 1, 0});     // replication only
    for (size_t i = 0; i < passes.size(); ++i) {
        const Pass &ps = passes[i];
        BfParams p;
        memset(&p, 0, sizeof(p));
        p.src = i == 0 ? src : dst;
        p.dst = dst;
        p.cache = cache;
        p.n_src = n_src;
        p.logn = logn; p.logrho = logrho;
        p.gather = (i == 0);
        p.c = ps.c; p.h = ps.h; p.A = ps.A; p.b_lo = ps.b_lo; p.b_hi = ps.b_hi;
        if (i + 1 == passes.size()) { p.scale = scale; p.sc_hi = sc_hi; p.sc_lo = sc_lo; p.final = 1; }
        const int tbits = ps.c + ps.A;
        const size_t lds = BN_BYTES << tbits;                                      // at most 64 KiB
        const size_t blocks = (size_t)1 << (logn - tbits);
        const int threads = (1 << tbits) >= 512 ? (1 << tbits) / 8 : 64;          // one radix-8 group per lane and step
        { ProfScope ps_("k_bn_mfft_pass", ((size_t)2 * BN_BYTES) << logn, (((size_t)1 << logn) >> 1) * (size_t)(ps.b_hi >= ps.b_lo ? ps.b_hi - ps.b_lo + 1 : 0));
          hipLaunchKernelGGL(k_bn_mfft_pass, dim3((unsigned)blocks), dim3(threads), lds, stream(), p); }
    }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

static int bn_ldt_grid(size_t n)
{
    size_t g = (n + 255) / 256;
    if (g > 8192) g = 8192;
    return (int)(g ? g : 1);
}

} // namespace iopx

using namespace iopx;

extern "C" {

int iopx_mul_fft_bn128_dev(const uint64_t *d_coeffs, size_t n_coeffs, size_t log_n, const uint64_t *gen,
                           const uint64_t *shift, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (log_n > (size_t)BN_TWO_ADICITY) return fail(IOPX_ERR_INVALID_ARGUMENT, "log_n %zu exceeds the 2-adicity of alt_bn128 Fr", log_n);
    if (!gen || !shift || !d_out || (n_coeffs && !d_coeffs)) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    const size_t n = (size_t)1 << log_n;
    if (n_coeffs > n) return fail(IOPX_ERR_INVALID_ARGUMENT, "multiplicative FFT: %zu coefficients exceed the domain size %zu", n_coeffs, n);
    if (n_coeffs == 0) return iopx::fill_bytes(d_out, 0, n * BN_BYTES);
    BnPlan *pl = nullptr;
    if ((rc = bn_get_plan((int)log_n, gen, &pl)) != IOPX_OK) return rc;
    if (!pl->have_fwd && (rc = bn_build_cache(*pl, false)) != IOPX_OK) return rc;
    const int logd = (int)ceil_log2(n_coeffs);
    const hbn sh = hbn::from_words(shift);
    if (sh.is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "multiplicative FFT: zero coset shift");
    TmpBuf scaled, hi, lo;
    const uint64_t *src = d_coeffs;
    if (d_coeffs == d_out) {    // the first pass permutes: it cannot run in place
        if ((rc = scaled.alloc(n_coeffs * BN_BYTES)) != IOPX_OK) return rc;
        if ((rc = iopx::copy_d2d(scaled.p, d_coeffs, n_coeffs * BN_BYTES)) != IOPX_OK) return rc;
        src = scaled.u64();
    }
    if (!(sh == hbn::one()) && n_coeffs > 1) {
        if (!scaled.p && (rc = scaled.alloc(n_coeffs * BN_BYTES)) != IOPX_OK) return rc;
        if ((rc = bn_build_two_level(sh, hbn::one(), logd, hi, lo)) != IOPX_OK) return rc;
        { ProfScope ps_("k_bn_scale_pow"); hipLaunchKernelGGL(k_bn_scale_pow, dim3(bgrid(n_coeffs, 256)), dim3(256), 0, stream(), scaled.u64(), src, (const uint64_t *)hi.u64(), (const uint64_t *)lo.u64(), n_coeffs); }
        src = scaled.u64();
    }
    return bn_run_mfft(pl->cache_fwd.u64(), src, n_coeffs, d_out, (int)log_n, (int)log_n - logd, 0, nullptr, nullptr);
}

int iopx_mul_ifft_bn128_dev(const uint64_t *d_evals, size_t log_n, const uint64_t *gen, const uint64_t *shift, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (log_n > (size_t)BN_TWO_ADICITY) return fail(IOPX_ERR_INVALID_ARGUMENT, "log_n %zu exceeds the 2-adicity of alt_bn128 Fr", log_n);
    if (!gen || !shift || !d_out || !d_evals) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    const size_t n = (size_t)1 << log_n;
    if (log_n == 0) return iopx::copy_d2d(d_out, d_evals, BN_BYTES);     // multiplicative_IFFT_wrapper returns {v[0]} (fft.tcc:397-401)
    BnPlan *pl = nullptr;
    if ((rc = bn_get_plan((int)log_n, gen, &pl)) != IOPX_OK) return rc;
    if (!pl->have_inv && (rc = bn_build_cache(*pl, true)) != IOPX_OK) return rc;
    const hbn sh = hbn::from_words(shift);
    if (sh.is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "multiplicative IFFT: zero coset shift");
    const hbn ninv = hbn::from_uint((uint64_t)n).inverse();
    TmpBuf hi, lo, tmp;
    int scale = 1;
    if (sh == hbn::one()) {
        if ((rc = hi.alloc(BN_BYTES)) != IOPX_OK) return rc;
        const hbn ninv_t = ninv.table_form();
        if ((rc = upload(hi.p, ninv_t.w, BN_BYTES)) != IOPX_OK) return rc;
    } else {
        scale = 2;       // out[i] *= n^-1 shift^-i
        if ((rc = bn_build_two_level(sh.inverse(), ninv, (int)log_n, hi, lo)) != IOPX_OK) return rc;
    }
    const uint64_t *src = d_evals;
    if (d_evals == d_out) {     // the first pass permutes: it cannot run in place
        if ((rc = tmp.alloc(n * BN_BYTES)) != IOPX_OK) return rc;
        if ((rc = iopx::copy_d2d(tmp.p, d_evals, n * BN_BYTES)) != IOPX_OK) return rc;
        src = tmp.u64();
    }
    return bn_run_mfft(pl->cache_inv.u64(), src, n, d_out, (int)log_n, 0, scale, hi.u64(), lo.p ? lo.u64() : nullptr);
}

int iopx_mul_ifft_known_degree_bn128_dev(const uint64_t *d_evals, size_t degree, size_t log_n, const uint64_t *gen,
                                         const uint64_t *shift, uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (log_n > (size_t)BN_TWO_ADICITY || degree == 0 || degree > ((size_t)1 << log_n)) return fail(IOPX_ERR_INVALID_ARGUMENT, "bad degree / domain size");
    if (!d_evals || !gen || !shift || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    const int k = (int)ceil_log2(degree);
    const size_t pow2 = (size_t)1 << k, stride = ((size_t)1 << log_n) >> k;
    TmpBuf sub;
    if ((rc = sub.alloc(pow2 * BN_BYTES)) != IOPX_OK) return rc;
    { ProfScope ps_("k_bn_gather_stride"); hipLaunchKernelGGL(k_bn_gather_stride, dim3(bgrid(4 * pow2, 256)), dim3(256), 0, stream(), sub.u64(), d_evals, stride, pow2); }
    IOPX_HIP(hipGetLastError());
    hbn gs = hbn::from_words(gen);          // generator of the sub-coset: g^(n / pow2)
    for (size_t s = stride; s > 1; s >>= 1) gs = gs.squared();
    return iopx_mul_ifft_bn128_dev(sub.u64(), (size_t)k, gs.w, shift, d_out);
}

int iopx_fri_fold_mul_bn128_dev(const uint64_t *d_f_i, size_t log_n, const uint64_t *gen, const uint64_t *shift,
                                size_t coset_size, const uint64_t *x_i, uint64_t *d_next)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (log_n > (size_t)BN_TWO_ADICITY) return fail(IOPX_ERR_INVALID_ARGUMENT, "log_n %zu exceeds the 2-adicity of alt_bn128 Fr", log_n);
    if (!d_f_i || !d_next || !gen || !shift || !x_i) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (coset_size == 0 || (coset_size & (coset_size - 1))) return fail(IOPX_ERR_INVALID_ARGUMENT, "coset size %zu is not a power of two", coset_size);
    const int eta = (int)ceil_log2(coset_size);
    if ((size_t)eta > log_n) return fail(IOPX_ERR_INVALID_ARGUMENT, "coset size %zu exceeds the domain size", coset_size);
    const size_t n = (size_t)1 << log_n;
    if (eta == 0) return iopx::copy_d2d(d_next, d_f_i, n * BN_BYTES);
    BnPlan *pl = nullptr;
    if ((rc = bn_get_plan((int)log_n, gen, &pl)) != IOPX_OK) return rc;
    if (!pl->have_inv && (rc = bn_build_cache(*pl, true)) != IOPX_OK) return rc;
    hbn sh = hbn::from_words(shift), x = hbn::from_words(x_i);
    if (sh.is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "FRI fold: zero coset shift");
    const hbn inv2 = hbn::from_uint(2).inverse().table_form();
    std::vector<uint64_t> hc;
    for (int e = 0; e < eta; ++e) {         // level e folds over the domain (shift^(2^e), g^(2^e)) at x^(2^e)
        const hbn xs = (x * sh.inverse()).table_form();
        hc.insert(hc.end(), xs.w, xs.w + 4);
        hc.insert(hc.end(), inv2.w, inv2.w + 4);
        sh = sh.squared();
        x = x.squared();
    }
    TmpBuf dc;
    if ((rc = dc.alloc(hc.size() * 8)) != IOPX_OK) return rc;
    if ((rc = upload(dc.p, hc.data(), hc.size() * 8)) != IOPX_OK) return rc;
    const uint64_t *ginv_top = pl->cache_inv.u64() + 4 * ((n >> 1) - 1);
    if (eta <= 3) {
        BfoldParams p;
        p.src = d_f_i; p.dst = d_next; p.ginv = ginv_top; p.consts = dc.u64(); p.half = n >> eta; p.stride_log = 0;
        const size_t bytes = (n + p.half) * BN_BYTES;
        if (eta == 1) { ProfScope ps_("k_bn_fri_fold_fused_eta1", bytes); hipLaunchKernelGGL(k_bn_fri_fold_fused<1>, dim3(bgrid(p.half, 256)), dim3(256), 0, stream(), p); }
        else if (eta == 2) { ProfScope ps_("k_bn_fri_fold_fused_eta2", bytes); hipLaunchKernelGGL(k_bn_fri_fold_fused<2>, dim3(bgrid(p.half, 256)), dim3(256), 0, stream(), p); }
        else { ProfScope ps_("k_bn_fri_fold_fused_eta3", bytes); hipLaunchKernelGGL(k_bn_fri_fold_fused<3>, dim3(bgrid(p.half, 256)), dim3(256), 0, stream(), p); }
        IOPX_HIP(hipGetLastError());
        return IOPX_OK;
    }
    TmpBuf tmp[2];
    const uint64_t *src = d_f_i;
    size_t cur = n;
    for (int e = 0; e < eta; ++e) {
        const size_t half = cur >> 1;
        uint64_t *dst = d_next;
        if (e != eta - 1) {
            if ((rc = tmp[e & 1].alloc(half * BN_BYTES)) != IOPX_OK) return rc;
            dst = tmp[e & 1].u64();
        }
        BfoldParams p;
        p.src = src; p.dst = dst; p.ginv = ginv_top; p.consts = dc.u64() + 8 * e; p.half = half; p.stride_log = e;
        { ProfScope ps_("k_bn_fri_fold2", (cur + half) * BN_BYTES); hipLaunchKernelGGL(k_bn_fri_fold2, dim3(bgrid(half, 256)), dim3(256), 0, stream(), p); }
        src = dst;
        cur = half;
    }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

int iopx_ldt_combine_bn128_dev(const void *const *d_oracles, size_t num_oracles, const size_t *degrees,
                               const uint64_t *random_coefficients, size_t log_n, const uint64_t *gen, const uint64_t *shift,
                               uint64_t *d_out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_oracles || !random_coefficients || !d_out || !gen || !shift) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (log_n > (size_t)BN_TWO_ADICITY) return fail(IOPX_ERR_INVALID_ARGUMENT, "log_n %zu exceeds the 2-adicity of alt_bn128 Fr", log_n);
    if (!degrees || num_oracles == 0) return fail(IOPX_ERR_INVALID_ARGUMENT, "Expected same number of evaluations as in registration.");
    // constructor + set_random_coefficients (ldt_reducer_aux.tcc:3-37): oracle k has its own coefficient c[k]; the i-th
    // submaximal one also c[num + i], times x^(max_degree - degree)
    size_t max_degree = 0;
    for (size_t k = 0; k < num_oracles; ++k) max_degree = degrees[k] > max_degree ? degrees[k] : max_degree;
    const hbn g = hbn::from_words(gen), s = hbn::from_words(shift);
    std::vector<uint64_t> hcoef;
    std::vector<std::unique_ptr<TmpBuf>> tabs;
    std::vector<const uint64_t *> hhi(num_oracles, nullptr), hlo(num_oracles, nullptr);
    size_t sub = 0;
    // coefficients_ = { 1 } followed by the random coefficients (set_random_coefficients, :25-37)
    auto coef = [&](size_t t) { return t ? hbn::from_words(random_coefficients + 4 * (t - 1)) : hbn::one(); };
    for (size_t k = 0; k < num_oracles; ++k) {
        const hbn a = coef(k).table_form();
        hcoef.insert(hcoef.end(), a.w, a.w + 4);
        if (degrees[k] == max_degree) continue;
        const uint64_t e = (uint64_t)(max_degree - degrees[k]);
        const hbn c2 = coef(num_oracles + sub);
        ++sub;
        // cur_bump_factor = c[num + i] * shift^e, multiplied by g^e per position (ldt_reducer_aux.tcc:112-126)
        tabs.emplace_back(new TmpBuf());
        tabs.emplace_back(new TmpBuf());
        TmpBuf &hi = *tabs[tabs.size() - 2], &lo = *tabs[tabs.size() - 1];
        if ((rc = bn_build_two_level(g.pow(e), c2 * s.pow(e), (int)log_n, hi, lo)) != IOPX_OK) return rc;
        hhi[k] = hi.u64();
        hlo[k] = lo.u64();
    }
    // one block: oracle pointers, the two table-pointer lists, the coefficients
    std::vector<uint64_t> meta(3 * num_oracles + hcoef.size());
    for (size_t k = 0; k < num_oracles; ++k) {
        meta[k] = (uint64_t)(uintptr_t)d_oracles[k];
        meta[num_oracles + k] = (uint64_t)(uintptr_t)hhi[k];
        meta[2 * num_oracles + k] = (uint64_t)(uintptr_t)hlo[k];
    }
    std::memcpy(&meta[3 * num_oracles], hcoef.data(), hcoef.size() * 8);
    TmpBuf dmeta;
    if ((rc = dmeta.alloc(meta.size() * 8)) != IOPX_OK) return rc;
    if ((rc = upload(dmeta.p, meta.data(), meta.size() * 8)) != IOPX_OK) return rc;
    BldtParams p;
    p.oracles = (const uint64_t *const *)dmeta.u64();
    p.hi = (const uint64_t *const *)(dmeta.u64() + num_oracles);
    p.lo = (const uint64_t *const *)(dmeta.u64() + 2 * num_oracles);
    p.out = d_out;
    p.coef = dmeta.u64() + 3 * num_oracles;
    p.n = (size_t)1 << log_n; p.num_oracles = (int)num_oracles;
    { ProfScope ps_("k_bn_ldt_combine", (num_oracles + 1) * p.n * BN_BYTES); hipLaunchKernelGGL(k_bn_ldt_combine, dim3(bn_ldt_grid(p.n)), dim3(256), 0, stream(), p); }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

// ---- host-side scalars (domain metadata of the template boundary; no device needed) ----
// multiplicative_subgroup_base::construct_internal (subgroup.tcc:55-59): multiplicative_generator^((r - 1) / 2^log_order)
int iopx_bn128_subgroup_generator(size_t log_order, uint64_t *gen)
{
    if (!gen) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (log_order > (size_t)BN_TWO_ADICITY) return fail(IOPX_ERR_INVALID_ARGUMENT, "log_order %zu exceeds the 2-adicity of alt_bn128 Fr", log_order);
    uint64_t e[4] = { hbn::P[0] - 1, hbn::P[1], hbn::P[2], hbn::P[3] };
    for (size_t s = 0; s < log_order; ++s) {
        for (int i = 0; i < 3; ++i) e[i] = (e[i] >> 1) | (e[i + 1] << 63);
        e[3] >>= 1;
    }
    const hbn g = hbn::from_uint(5).pow_limbs(e, 4);
    memcpy(gen, g.w, BN_BYTES);
    return IOPX_OK;
}
int iopx_bn128_multiplicative_generator(uint64_t *gen)        // libff alt_bn128_Fr::multiplicative_generator = 5
{
    if (!gen) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    const hbn g = hbn::from_uint(5);
    memcpy(gen, g.w, BN_BYTES);
    return IOPX_OK;
}
int iopx_bn128_from_uint(uint64_t v, uint64_t *out)            // FieldT(v)
{
    if (!out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    const hbn r = hbn::from_uint(v);
    memcpy(out, r.w, BN_BYTES);
    return IOPX_OK;
}
int iopx_bn128_host_mul(const uint64_t *a, const uint64_t *b, uint64_t *out)
{
    if (!a || !b || !out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    const hbn r = hbn::from_words(a) * hbn::from_words(b);
    memcpy(out, r.w, BN_BYTES);
    return IOPX_OK;
}
int iopx_bn128_host_pow(const uint64_t *a, uint64_t exponent, uint64_t *out)
{
    if (!a || !out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    const hbn r = hbn::from_words(a).pow(exponent);
    memcpy(out, r.w, BN_BYTES);
    return IOPX_OK;
}
int iopx_bn128_host_inverse(const uint64_t *a, uint64_t *out)
{
    if (!a || !out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    const hbn x = hbn::from_words(a);
    if (x.is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "inverse of zero");
    const hbn r = x.inverse();
    memcpy(out, r.w, BN_BYTES);
    return IOPX_OK;
}

// ---- host-pointer variants ---------------------------------------------------------------------
int iopx_mul_fft_bn128(const uint64_t *coeffs, size_t n_coeffs, size_t log_n, const uint64_t *gen, const uint64_t *shift, uint64_t *out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (log_n > (size_t)BN_TWO_ADICITY) return fail(IOPX_ERR_INVALID_ARGUMENT, "log_n %zu exceeds the 2-adicity of alt_bn128 Fr", log_n);
    if (!out || (n_coeffs && !coeffs)) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    const size_t n = (size_t)1 << log_n;
    if (n_coeffs > n) return fail(IOPX_ERR_INVALID_ARGUMENT, "multiplicative FFT: %zu coefficients exceed the domain size %zu", n_coeffs, n);
    DevBuf din, dout;
    if ((rc = din.alloc(n_coeffs * BN_BYTES)) != IOPX_OK) return rc;
    if ((rc = dout.alloc(n * BN_BYTES)) != IOPX_OK) return rc;
    if (n_coeffs) IOPX_HIP(copy_h2d(din.p, coeffs, n_coeffs * BN_BYTES, stream()));
    if ((rc = iopx_mul_fft_bn128_dev(din.u64(), n_coeffs, log_n, gen, shift, dout.u64())) != IOPX_OK) return rc;
    IOPX_HIP(copy_d2h(out, dout.p, n * BN_BYTES, stream()));
    IOPX_HIP(hipStreamSynchronize(stream()));
    return IOPX_OK;
}

int iopx_mul_ifft_bn128(const uint64_t *evals, size_t log_n, const uint64_t *gen, const uint64_t *shift, uint64_t *out)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (log_n > (size_t)BN_TWO_ADICITY) return fail(IOPX_ERR_INVALID_ARGUMENT, "log_n %zu exceeds the 2-adicity of alt_bn128 Fr", log_n);
    if (!evals || !out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    const size_t n = (size_t)1 << log_n;
    DevBuf din, dout;
    if ((rc = din.alloc(n * BN_BYTES)) != IOPX_OK) return rc;
    if ((rc = dout.alloc(n * BN_BYTES)) != IOPX_OK) return rc;
    IOPX_HIP(copy_h2d(din.p, evals, n * BN_BYTES, stream()));
    if ((rc = iopx_mul_ifft_bn128_dev(din.u64(), log_n, gen, shift, dout.u64())) != IOPX_OK) return rc;
    IOPX_HIP(copy_d2h(out, dout.p, n * BN_BYTES, stream()));
    IOPX_HIP(hipStreamSynchronize(stream()));
    return IOPX_OK;
}

int iopx_fri_fold_mul_bn128(const uint64_t *f_i, size_t log_n, const uint64_t *gen, const uint64_t *shift, size_t coset_size,
                            const uint64_t *x_i, uint64_t *next)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (log_n > (size_t)BN_TWO_ADICITY) return fail(IOPX_ERR_INVALID_ARGUMENT, "log_n %zu exceeds the 2-adicity of alt_bn128 Fr", log_n);
    if (!f_i || !next) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (coset_size == 0 || (coset_size & (coset_size - 1)) || coset_size > ((size_t)1 << log_n))
        return fail(IOPX_ERR_INVALID_ARGUMENT, "bad coset size %zu", coset_size);
    const size_t n = (size_t)1 << log_n, n_out = n / coset_size;
    DevBuf din, dout;
    if ((rc = din.alloc(n * BN_BYTES)) != IOPX_OK) return rc;
    if ((rc = dout.alloc(n_out * BN_BYTES)) != IOPX_OK) return rc;
    IOPX_HIP(copy_h2d(din.p, f_i, n * BN_BYTES, stream()));
    if ((rc = iopx_fri_fold_mul_bn128_dev(din.u64(), log_n, gen, shift, coset_size, x_i, dout.u64())) != IOPX_OK) return rc;
    IOPX_HIP(copy_d2h(next, dout.p, n_out * BN_BYTES, stream()));
    IOPX_HIP(hipStreamSynchronize(stream()));
    return IOPX_OK;
}

} // extern "C"
