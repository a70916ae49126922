// alt_bn128 Fr (r = 21888242871839275222246405745257275088548364400416034343698204186575808495617) in radix 2^29 for
// gfx950: shared by the Poseidon kernels (poseidon_bn128.hip) and the multiplicative FFT / FRI fold (fft_mul.hip) and LDT
// combination (ldt_reducer.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace iopx {

// ---- alt_bn128 Fr in radix 2^29 ----------------------------------------------------------------------------------
// gfx950's widest integer multiply is v_mad_u64_u32 (32 x 32 + 64 -> 64, no carry-in).  Nine 29-bit limbs leave enough
// headroom in that 64-bit accumulator for a whole column of a Montgomery product (nine a_i * b_j and nine m_i * p_j
// terms), so a product is 162 multiply-adds and no carry chains; additions are limb-wise with no carries at all.
// Internally an element x is any representative of x * 2^261 mod p below 2^257.5 ("R261 form"); the library's
// boundary stays libff's 4 x 64-bit Montgomery words (x * 2^256 mod p, canonical), converted on load / store.
struct bn9 {
    uint32_t l[9];
};

#define BN9_MASK 0x1fffffffu
__device__ static const uint32_t BN9_P[9] = { 0x10000001u, 0x1f0fac9fu, 0x0e5c2450u, 0x07d090f3u, 0x1585d283u, 0x02db40c0u, 0x00a6e141u, 0x0e5c2634u, 0x0030644eu };
#define BN9_INV 0x0fffffffu                  // -p^-1 mod 2^29
// 2^e mod p as plain 29-bit limbs: multiplying by them (one Montgomery product, / 2^261) moves between the forms
__device__ static const uint32_t BN9_C256[9] = { 0x0ffffffbu, 0x04b1a0e2u, 0x18334a6bu, 0x18ed2b3eu, 0x1462e36fu, 0x11b7bc3cu, 0x1cbd99bau, 0x183340fbu, 0x000e0a77u };
__device__ static const uint32_t BN9_C266[9] = { 0x0fffead7u, 0x1d5444f4u, 0x04438aa5u, 0x03b4d096u, 0x134c84dau, 0x0e92d304u, 0x14cb95b3u, 0x041b9d3du, 0x00058003u };
__device__ static const uint32_t BN9_C517[9] = { 0x142db4dfu, 0x19d6990eu, 0x1472f48cu, 0x06dbe7e3u, 0x0b84d579u, 0x10f9faf7u, 0x121f4380u, 0x17a112deu, 0x001275c7u };
__device__ static const uint32_t BN9_C522[9] = { 0x05b69bd4u, 0x06170a5au, 0x020cddceu, 0x1db6310bu, 0x0e54d0ffu, 0x1cf855e3u, 0x1c15e103u, 0x07d09161u, 0x000a054au };
__device__ static const uint32_t BN_P32[8] = { 0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u };

__device__ __forceinline__ bn9 bn9_const(const uint32_t (&c)[9])
{
    bn9 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = c[i];
    return r;
}

__device__ __forceinline__ bn9 bn9_zero()
{
    bn9 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = 0;
    return r;
}

// 256-bit integer (4 little-endian 64-bit words) -> nine 29-bit limbs
__device__ __forceinline__ bn9 bn9_unpack(const uint64_t *q)
{
    uint32_t w[9];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const uint64_t v = q[i]; w[2 * i] = (uint32_t)v; w[2 * i + 1] = (uint32_t)(v >> 32); }
    w[8] = 0;
    bn9 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int bit = 29 * i, wi = bit >> 5, sh = bit & 31;
        const uint64_t two = (uint64_t)w[wi] | ((uint64_t)w[wi + 1 > 8 ? 8 : wi + 1] << 32);
        r.l[i] = (uint32_t)(two >> sh) & BN9_MASK;
    }
    return r;
}

// limb-wise sum; no carries (see the headroom rules at bn9_mul)
__device__ __forceinline__ bn9 bn9_add(const bn9 &a, const bn9 &b)
{
    bn9 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = a.l[i] + b.l[i];
    return r;
}

// carry propagation: same value, limbs 0..7 back below 2^29
__device__ __forceinline__ bn9 bn9_norm(const bn9 &a)
{
    bn9 r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t v = a.l[i] + c;
        r.l[i] = v & BN9_MASK;
        c = v >> 29;
    }
    r.l[8] = a.l[8] + c;
    return r;
}

// 2^254 - p, plain limbs: v = q * 2^254 + rem is congruent to q * (2^254 - p) + rem
__device__ static const uint32_t BN9_C254[9] = { 0x0fffffffu, 0x00f05360u, 0x11a3dbafu, 0x182f6f0cu, 0x0a7a2d7cu, 0x1d24bf3fu, 0x1f591ebeu, 0x11a3d9cbu, 0x000f9bb1u };

// Weak reduction of a limb vector (limbs 0..7 up to 2^32 - 8: bn9_norm adds a carry of up to 7 in 32 bits): same residue, value below 2^254 + (v >> 254) * 0.25 * 2^254 and
// normalised limbs.  Used where elements are only ever added (the near-MDS layers), so that they stay below 2^256.
__device__ __forceinline__ bn9 bn9_reduce(const bn9 &a)
{
    bn9 n = bn9_norm(a);
    const uint32_t q = n.l[8] >> 22;
    n.l[8] &= 0x3fffffu;
    bn9 r;
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        acc += (uint64_t)q * BN9_C254[i] + n.l[i];
        r.l[i] = (uint32_t)acc & BN9_MASK;
        acc >>= 29;
    }
    r.l[8] = (uint32_t)acc + q * BN9_C254[8] + n.l[8];
    return r;
}

// Montgomery reduction interleaved with the column sums (product scanning).  On entry to column k `acc` holds the
// carry of column k - 1; COLUMN(k) adds the operand products, then the m_i * p_j terms.
#define BN9_REDUCE_LOW(k)                                                                 \
    {                                                                                     \
        _Pragma("unroll") for (int i = 0; i < (k); ++i) acc += (uint64_t)m[i] * BN9_P[(k) - i]; \
        m[k] = ((uint32_t)acc * BN9_INV) & BN9_MASK;                                      \
        acc += (uint64_t)m[k] * BN9_P[0];                                                 \
        acc >>= 29;                                                                       \
    }
#define BN9_REDUCE_HIGH(k)                                                                \
    {                                                                                     \
        _Pragma("unroll") for (int i = (k) - 8; i < 9; ++i) acc += (uint64_t)m[i] * BN9_P[(k) - i]; \
        r.l[(k) - 9] = (uint32_t)acc & BN9_MASK;                                          \
        acc >>= 29;                                                                       \
    }

// sum_n a[n] * b[n] * 2^-261 mod p for N operand pairs reduced together.
// Headroom: every column must stay below 2^64, i.e. N * 9 * max(a limb) * max(b limb) + 9 * 2^58 < 2^64:
//   N = 1: both operands may have limbs up to 2^30 (one carry-less addition each), or one up to 2^31 against a normalised one;
//   N = 3: one side normalised (< 2^29), the other up to 2^30;   N = 4: both normalised.
// Values: inputs below 2^257.5 give a result below 2^255 with normalised limbs.
template<int N>
__device__ __forceinline__ bn9 bn9_dot(const bn9 (&a)[N], const bn9 (&b)[N])
{
    uint32_t m[9];
    bn9 r;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
#pragma unroll
        for (int n = 0; n < N; ++n) {
#pragma unroll
            for (int i = 0; i <= k; ++i) acc += (uint64_t)a[n].l[i] * b[n].l[k - i];
        }
        BN9_REDUCE_LOW(k)
    }
#pragma unroll
    for (int k = 9; k < 17; ++k) {
#pragma unroll
        for (int n = 0; n < N; ++n) {
#pragma unroll
            for (int i = k - 8; i < 9; ++i) acc += (uint64_t)a[n].l[i] * b[n].l[k - i];
        }
        BN9_REDUCE_HIGH(k)
    }
    r.l[8] = (uint32_t)acc;
    return r;
}

__device__ __forceinline__ bn9 bn9_mul(const bn9 &a, const bn9 &b)
{
    const bn9 aa[1] = { a }, bb[1] = { b };
    return bn9_dot<1>(aa, bb);
}

// a * a * 2^-261: the cross terms once, against the doubled operand (45 products instead of 81); limbs of a up to 2^30
__device__ __forceinline__ bn9 bn9_sqr(const bn9 &a)
{
    uint32_t m[9], d[9];
    bn9 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) d[i] = a.l[i] << 1;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
#pragma unroll
        for (int i = 0; 2 * i < k; ++i) acc += (uint64_t)a.l[i] * d[k - i];
        if ((k & 1) == 0) acc += (uint64_t)a.l[k / 2] * a.l[k / 2];
        BN9_REDUCE_LOW(k)
    }
#pragma unroll
    for (int k = 9; k < 17; ++k) {
#pragma unroll
        for (int i = k - 8; 2 * i < k; ++i) acc += (uint64_t)a.l[i] * d[k - i];
        if ((k & 1) == 0) acc += (uint64_t)a.l[k / 2] * a.l[k / 2];
        BN9_REDUCE_HIGH(k)
    }
    r.l[8] = (uint32_t)acc;
    return r;
}

// libff words (x * 2^256, canonical) -> R261 form
__device__ __forceinline__ bn9 bn9_load_mont(const uint64_t *p, size_t idx)
{
    return bn9_mul(bn9_unpack(p + 4 * idx), bn9_const(BN9_C266));
}

// value below 2r with normalised limbs (a product of a value below 2^256 and a canonical one) -> canonical 4 x 64-bit words: r is subtracted once
__device__ __forceinline__ void bn9_store_canonical(uint64_t *q, const bn9 &y)
{
    uint32_t w[8], d[8];
    uint64_t acc = 0;
    int bits = 0, wi = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        acc |= (uint64_t)y.l[i] << bits;
        bits += 29;
        if (bits >= 32 && wi < 8) { w[wi++] = (uint32_t)acc; acc >>= 32; bits -= 32; }
    }
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t t = (uint64_t)w[i] - BN_P32[i] - borrow;
        d[i] = (uint32_t)t;
        borrow = (t >> 32) & 1;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lo = borrow ? w[2 * i] : d[2 * i], hi = borrow ? w[2 * i + 1] : d[2 * i + 1];
        q[i] = (uint64_t)lo | ((uint64_t)hi << 32);
    }
}

// R261 form (any representative) -> libff words
__device__ __forceinline__ void bn9_store_mont(uint64_t *p, size_t idx, const bn9 &x)
{
    bn9_store_canonical(p + 4 * idx, bn9_mul(x, bn9_const(BN9_C256)));
}

// ---- weak values in the library's x * 2^256 form: the multiplicative-coset kernels (fft_mul.hip, ldt_reducer.hip) ------
// Elements are libff Fp_model<4> Montgomery words (x * 2^256 mod r, four little-endian uint64, canonical at the boundary).
// Those kernels keep data in that form throughout and every multiplier (twiddles, shift powers, n^-1, 1/2, fold and LDT
// constants) in "table form" t * 2^261 (hbn::table_form), so x 2^256 * t 2^261 / 2^261 = x t 2^256 and no conversion is ever
// needed.  Between operations a value is any representative below 2^256 with normalised limbs ("weak"); sums and differences
// are brought back below 2^256 by bn9_reduce, products of weak values are below 2r.  Kernels store canonical words.

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

// ---- helpers of the protocol-layer kernels (virtual_oracles.hip, encoded_ops.hip, fractal_ops.hip) ----------------------
// Those kernels are the first to multiply DATA by DATA: x 2^256 * y 2^256 / 2^261 = x y 2^251.  The other terms of the same sum are
// brought to that scale inside one bn9_dot (times the stored 1 = 2^256, or times BN9_C261 = the table form of 1 when the sum
// stays in the data form), and a constant the host uploads anyway carries the missing 2^5 (table_form() applied twice: t 2^266).

// -b as limbs: 8r - b, limb-wise non-negative for a weak b; limbs below 2^30, value below 2^257 (an operand of bn9_dot / bn9_mul)
__device__ __forceinline__ bn9 bn9_negw(const bn9 &b)
{
    bn9 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = BN9_8R[i] - b.l[i];
    return r;
}

// whether a raw 256-bit word (normalised limbs) is a multiple of r: 0, r, ..., 5r are the ones below 2^256 (constants fold)
__device__ __forceinline__ bool bn9_is_zero_mod(const bn9 &x)
{
    bool z = false;
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {
        bool eq = true;
        uint32_t carry = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const uint32_t v = k * BN9_P[i] + carry;        // below 6 * 2^29: fits
            eq = eq && x.l[i] == (i < 8 ? (v & BN9_MASK) : v);
            carry = v >> 29;
        }
        z = z || eq;
    }
    return z;
}

// x^(r-2) for x in the 2^261 form (closed under bn9_mul / bn9_sqr); e: the four raw words of r - 2, whose top bit is bit 253.
// 253 squarings and 127 products: shared by a whole batch through Montgomery's trick, never paid per element.
__device__ __forceinline__ bn9 bn9_fermat_inverse(const bn9 &x, const uint64_t *e)
{
    bn9 r = x;
#pragma unroll 1
    for (int bit = 252; bit >= 0; --bit) {
        r = bn9_sqr(r);
        if ((e[bit >> 6] >> (bit & 63)) & 1) r = bn9_mul(r, x);
    }
    return r;
}

template<int N, class LoadA, class LoadB>
__device__ __forceinline__ bn9 bn9_dot_loaded(LoadA la, LoadB lb, size_t g)
{
    bn9 a[N], b[N];
#pragma unroll
    for (int i = 0; i < N; ++i) { a[i] = la(g + i); b[i] = lb(g + i); }
    return bn9_dot<N>(a, b);
}

// sum_{begin <= t < end} la(t) * lb(t) * 2^-261 as a weak value: four products per reduction (bn9_dot's headroom for normalised
// operands), the groups added up; la / lb yield weak values.  An empty range gives zero.
template<class LoadA, class LoadB>
__device__ __forceinline__ bn9 bn9_sum_products(LoadA la, LoadB lb, size_t begin, size_t end)
{
    bn9 acc = bn9_zero();
    bool have = false;
    for (size_t g = begin; g < end; g += 4) {
        const size_t k = end - g;
        bn9 t;
        if (k >= 4) t = bn9_dot_loaded<4>(la, lb, g);
        else if (k == 3) t = bn9_dot_loaded<3>(la, lb, g);
        else if (k == 2) t = bn9_dot_loaded<2>(la, lb, g);
        else t = bn9_dot_loaded<1>(la, lb, g);
        acc = have ? bnw_add(acc, t) : t;
        have = true;
    }
    return acc;
}

} // namespace iopx
