// The additive arm over a binary field on gfx950, written once: additive FFT / IFFT / low-degree extension, FRI fold and domain chain,
// LDT combination, vector helpers — kernels, host driver and the bodies of the C entries.  gf64.hip, gf128.hip and gf256.hip include this
// text and instantiate it for their element trait.
//
// The transforms replace additive_FFT / additive_IFFT of the reference (libiop/algebra/fft.tcc:39-124, 126-204) in two phases:
//
//   phase 1  (coefficients -> Gao–Mateer basis), in place on 2^d elements, d = ceil(log2 n_coeffs): per level j the twist by
//            beta_j^(idx >> j) (power table in HBM, built once per basis) and the Taylor-expansion XOR network on index bits (k+1, k),
//            k = d-2 .. j (fft.tcc:62-83), in LDS tiles of 2^c contiguous columns x 2^A rows on consecutive index bits;
//   phase 2  (the unwind butterflies, fft.tcc:102-120) without the bit reversal of fft.tcc:99: pair bit p = d-1 .. 0 in block order, the
//            bit reversal folded into the addressing of the last pass.  It runs once per coset of span(basis[0..d)): the twiddles of two
//            cosets differ by a per-level additive constant (the recursed shift is GF(2)-linear in the coset shift).
//
// A tile of 2^T elements carries T - c butterfly levels per upper pass and the low T - c_top levels + the bit reversal in the last one
// (schedule_x); the pass structure does not depend on the element's width, only T does.  No wave-uniform multiplier form is used: the
// general product is issued per element.  The IFFT runs the exact inverse schedule.
//
// An element trait F gives
//   W, mem (the form in HBM and LDS), reg, load<A16> / store<A16>, zero, one, add, unpack, pack, rmul, mul, inv                        (device)
//   host (the portable twin: construction from words, store, is_zero, +, *, squared, inverse, zero, one)                               (host)
//   stem() (the profile-name stem), option(i) (the four tile options' names), TILE_DEFAULT / TILE_MAX / P1_COLS_DEFAULT / P2_COLS_DEFAULT / P2_TOP_DEFAULT,
//   UPPER_WAVES (the occupancy the upper butterfly passes are bounded to), STAGE_BITS (log2 of the elements the block-order staging of
//   an LDE's coset group may hold), SPLIT_ACCESS (below), cold_plan() / cold_pow() (cold-cost labels), LDT_TAG, CACHE_BYTES (the bound
//   of the plan cache).
// The C ABI hands arrays over as uint64_t *: they are 8-byte aligned and no more.  Where an element is wider than that (SPLIT_ACCESS), every
// kernel has two instantiations: A16 (128-bit accesses) is launched only when the host has found every pointer of the launch 16-byte
// aligned, the other one reads and writes an element as 64-bit words.  The profile tells them apart: the 64-bit instantiation reports under
// the kernel's name with "_w64" appended.  A one-word element has the 64-bit instantiation alone, under the plain name.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "runtime.h"
#include "subspace_poly.h"

namespace iopx {

// Tile geometry: options of runtime.h's table, looked up when a plan is built (a plan keeps the geometry it was built with and the plan key
// carries it).  The tests set small values with iopx_set_option to reach the multi-pass schedules at small transform sizes.
struct TuningX { int tile_bits, p1_cols, p2_cols, p2_top; };
template<class F>
static TuningX tuning_x()
{
    TuningX u;
    u.tile_bits = opt_range(F::option(0), F::TILE_DEFAULT, 3, F::TILE_MAX);            // 2^tile_bits elements of LDS
    u.p1_cols = opt_range(F::option(1), F::P1_COLS_DEFAULT, 0, u.tile_bits - 2);       // phase-1 tiles: 2^c contiguous columns
    u.p2_cols = opt_range(F::option(2), F::P2_COLS_DEFAULT, 0, u.tile_bits - 2);       // phase-2 upper tiles
    u.p2_top = opt_range(F::option(3), F::P2_TOP_DEFAULT, 0, u.tile_bits - 2);         // last pass: 2^top natural-order runs
    return u;
}

static int grid_x(size_t work, int threads)
{
    size_t g = (work + threads - 1) / threads;
    if (g > 16384) g = 16384;
    return (int)(g ? g : 1);
}

static bool al16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// the profile name of a kernel: the field's stem + the kernel's name (+ "_w64"); built once per name, the pointer stays valid
template<class F>
static const char *kernel_name(const char *kernel, bool w64)
{
    static std::mutex mu;
    static std::map<std::string, std::string> names[2];
    std::lock_guard<std::mutex> lk(mu);
    std::string &s = names[w64 ? 1 : 0][kernel];
    if (s.empty()) s = std::string(F::stem()) + kernel + (w64 ? "_w64" : "");
    return s.c_str();
}

// launch the A16 instantiation when `a16`, the 64-bit one otherwise, under the matching profile name; a field without the split has
// (and names) the 64-bit one only
#define IOPX_LAUNCHX(a16, name, bytes, K, grid, threads, lds, ...)                                                     \
    do {                                                                                                               \
        const bool a16_ = (a16);                                                                                       \
        ProfScope ps_(kernel_name<F>(name, F::SPLIT_ACCESS && !a16_), bytes);                                          \
        if constexpr (F::SPLIT_ACCESS) {                                                                               \
            if (a16_) hipLaunchKernelGGL((K<F, true>), grid, threads, lds, stream(), __VA_ARGS__);                     \
            else hipLaunchKernelGGL((K<F, false>), grid, threads, lds, stream(), __VA_ARGS__);                         \
        } else {                                                                                                       \
            hipLaunchKernelGGL((K<F, false>), grid, threads, lds, stream(), __VA_ARGS__);                              \
        }                                                                                                              \
    } while (0)

__device__ __forceinline__ uint32_t bitrev_low(uint32_t x, int bits)
{
    return bits == 0 ? 0u : (__brev(x) >> (32 - bits));
}

// ---------------------------------------------------------------------------------------------
// plan construction, padding
// ---------------------------------------------------------------------------------------------
// out[q] = prod_{k : bit k of q} sq[k]  for q < count   (sq[k] = beta^(2^k))
template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_pow_direct(uint64_t *out, const uint64_t *sq, int nbits, size_t count)
{
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < count; q += (size_t)gridDim.x * blockDim.x) {
        typename F::reg acc = F::unpack(F::one());
        for (int k = 0; k < nbits; ++k) {
            if ((q >> k) & 1) acc = F::rmul(acc, F::unpack(F::template load<A16>(sq, k)));
        }
        F::template store<A16>(out, q, F::pack(acc));
    }
}

// Twiddle table in block order: pair bit p owns the 2^(d-1-p) entries at offset 2^(d-1-p) - 1; entry t is sum_k bit_{l-1-k}(t) * B_p[k],
// l = d-1-p, B_p = the l recursed basis vectors of recursion level p (fft.tcc:87-92, popped at :104-110) — sums[rev_l(t)] without the shift term.
template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_build_ltab(uint64_t *ltab, const uint64_t *rec_betas, int d, size_t count)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (size_t)gridDim.x * blockDim.x) {
        int l = 0;
        while (((size_t)2 << l) <= e + 1) ++l;          // l = floor(log2(e + 1))
        const size_t t = e + 1 - ((size_t)1 << l);
        const int p = d - 1 - l;
        const size_t off = (size_t)p * (d - 1) - (size_t)p * (p - 1) / 2;       // level p has d-1-p entries, levels back to back
        typename F::mem acc = F::zero();
        for (int k = 0; k < l; ++k) {
            if ((t >> (l - 1 - k)) & 1) acc = F::add(acc, F::template load<A16>(rec_betas, off + k));
        }
        F::template store<A16>(ltab, e, acc);
    }
}

template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_pad_copy(uint64_t *dst, const uint64_t *src, size_t n_src, size_t n_dst)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_dst; i += (size_t)gridDim.x * blockDim.x)
        F::template store<A16>(dst, i, i < n_src ? F::template load<A16>(src, i) : F::zero());
}

// out[i] = c for every i (degree-0 polynomial: n_coeffs <= 1)
template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_fill(uint64_t *dst, const uint64_t *src, int have_src, size_t n)
{
    const typename F::mem a = have_src ? F::template load<A16>(src, 0) : F::zero();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) F::template store<A16>(dst, i, a);
}

// ---------------------------------------------------------------------------------------------
// phase 1: twist + Taylor-expansion network on an LDS tile
// ---------------------------------------------------------------------------------------------
struct P1ParamsX {
    uint64_t *S;            // 2^d elements, updated in place
    const uint64_t *pow;    // power tables, level j at element offset 2^(d+1) - 2^(d+1-j), 2^(d-j) entries (inverse: powers of 1 / beta_j)
    int d;
    int c, h, A;            // tile = columns on bits [0,c) x rows on bits [h, h+A)
    int j0, j1;             // levels handled by this pass
    int k_start, k_end;     // first op of level j0, last op of level j1 (ops run k = d-2 .. j)
    int twist_first;        // 1: level j0's twist belongs to this pass (the levels after j0 always bring theirs)
};

template<class F, bool A16, bool INV>
__device__ __forceinline__ void phase1_body(const P1ParamsX &p)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t iopx_smem[];
    typename F::mem *s = reinterpret_cast<typename F::mem *>(iopx_smem);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int E = 1 << (p.c + p.A);
    const int midbits = p.h - p.c;
    const size_t o = blockIdx.x;
    const size_t mid = o & (((size_t)1 << midbits) - 1), hi = o >> midbits;
    const size_t base = (hi << (p.h + p.A)) | (mid << p.c);
    const int cmask = (1 << p.c) - 1;

    for (int li = tid; li < E; li += nt) s[li] = F::template load<A16>(p.S, base | ((size_t)(li >> p.c) << p.h) | (size_t)(li & cmask));
    __syncthreads();

    const int jb = INV ? p.j1 : p.j0, je = INV ? p.j0 - 1 : p.j1 + 1, js = INV ? -1 : 1;
    for (int j = jb; j != je; j += js) {
        const int ks = (j == p.j0) ? p.k_start : p.d - 2;
        const int ke = (j == p.j1) ? p.k_end : j;
        const bool twist = (j > p.j0) || p.twist_first;
        const uint64_t *powj = p.pow + (size_t)F::W * ((((size_t)2) << p.d) - (((size_t)2) << (p.d - j)));
        if (!INV && twist) {
            for (int li = tid; li < E; li += nt) {
                const size_t gi = base | ((size_t)(li >> p.c) << p.h) | (size_t)(li & cmask);
                s[li] = F::mul(s[li], F::template load<A16>(powj, gi >> j));
            }
            __syncthreads();
        }
        const int nops = ks - ke + 1;                   // forward: k = ks down to ke; inverse: k = ke up to ks
        for (int t = 0; t < nops; ++t) {
            const int k = INV ? ke + t : ks - t;
            const int kl = k - p.h + p.c;               // tile-local bit of global bit k
            for (int qd = tid; qd < (E >> 2); qd += nt) {
                const int low = qd & ((1 << kl) - 1), high = qd >> kl;
                const int b0 = (high << (kl + 2)) | low;
                const int e1 = b0 | (1 << kl), e2 = b0 | (2 << kl), e3 = b0 | (3 << kl);
                if (!INV) {                             // S[2s+i] += S[3s+i]; S[s+i] += S[2s+i]            (fft.tcc:79-80)
                    const typename F::mem v2 = F::add(s[e2], s[e3]);
                    s[e2] = v2;
                    s[e1] = F::add(s[e1], v2);
                } else {                                // S[q+i] += S[2q+i]; S[2q+i] += S[3q+i]            (fft.tcc:183-184)
                    const typename F::mem v2 = s[e2];
                    s[e1] = F::add(s[e1], v2);
                    s[e2] = F::add(v2, s[e3]);
                }
            }
            __syncthreads();
        }
        if (INV && twist) {
            for (int li = tid; li < E; li += nt) {
                const size_t gi = base | ((size_t)(li >> p.c) << p.h) | (size_t)(li & cmask);
                s[li] = F::mul(s[li], F::template load<A16>(powj, gi >> j));
            }
            __syncthreads();
        }
    }

    for (int li = tid; li < E; li += nt) F::template store<A16>(p.S, base | ((size_t)(li >> p.c) << p.h) | (size_t)(li & cmask), s[li]);
}

template<class F, bool A16> __global__ void __launch_bounds__(512) kx_phase1(P1ParamsX p) { phase1_body<F, A16, false>(p); }
template<class F, bool A16> __global__ void __launch_bounds__(512) kx_phase1_inv(P1ParamsX p) { phase1_body<F, A16, true>(p); }

// ---------------------------------------------------------------------------------------------
// phase 2: butterflies in block order
// ---------------------------------------------------------------------------------------------
struct BfParamsX {
    const uint64_t *src;    // forward: W (2^d, shared by all cosets) when src_shared, else the layout of dst
    uint64_t *dst;          // cosets * 2^d elements
    const uint64_t *ltab;   // 2^d - 1 twiddles (no shift term)
    const uint64_t *rs;     // (1 + nhi) * d shift terms: rs[v * d + p], v = 0 the shift, v = 1 + k coset basis vector k
    int src_shared;
    int d, nhi;
    int c, h, A;            // upper pass tile geometry
    int p_hi, p_lo;         // pair bits handled (forward: p_hi down to p_lo)
    int a_low, c_top;       // last/first pass tile: low a_low bits x top c_top bits
    int g_bits;             // last/first pass: 2^g_bits tiles per workgroup
    size_t total_units;     // cosets (of this launch) * tiles per coset
    size_t coset_base;      // global index of the first coset of this launch (src/dst are pre-offset)
};

// shift term of the twiddles of pair bit pbit in coset `coset` of the launch
template<class F, bool A16>
__device__ __forceinline__ typename F::mem bf_shift_term(const BfParamsX &p, size_t coset, int pbit)
{
    const size_t gc = p.coset_base + coset;
    typename F::mem tw = F::template load<A16>(p.rs, pbit);
    for (int v = 0; v < p.nhi; ++v) {
        if ((gc >> v) & 1) tw = F::add(tw, F::template load<A16>(p.rs, (size_t)(1 + v) * p.d + pbit));
    }
    return tw;
}

template<class F, bool INV>
__device__ __forceinline__ void bf_apply(typename F::mem *s, int ia, int ib, const typename F::mem &tw)
{
    typename F::mem a = s[ia], b = s[ib];
    if (!INV) {
        a = F::add(a, F::mul(b, tw));                   // S[a] += S[b] * t ; S[b] += S[a]  (fft.tcc:116-117)
        b = F::add(b, a);
    } else {
        b = F::add(b, a);                               // S[b] += S[a] ; S[a] += S[b] * t  (fft.tcc:164-165)
        a = F::add(a, F::mul(b, tw));
    }
    s[ia] = a;
    s[ib] = b;
}

template<class F, bool A16, bool INV>
__device__ __forceinline__ void bfly_upper_body(const BfParamsX &p)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t iopx_smem[];
    typename F::mem *s = reinterpret_cast<typename F::mem *>(iopx_smem);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int E = 1 << (p.c + p.A);
    const int tpc_bits = p.d - p.c - p.A;
    const size_t unit = blockIdx.x;
    const size_t coset = unit >> tpc_bits, o = unit & (((size_t)1 << tpc_bits) - 1);
    const int midbits = p.h - p.c;
    const size_t mid = o & (((size_t)1 << midbits) - 1), hi = o >> midbits;
    const size_t base = (hi << (p.h + p.A)) | (mid << p.c);
    const int cmask = (1 << p.c) - 1;
    const uint64_t *src = p.src_shared ? p.src : p.src + (size_t)F::W * (coset << p.d);
    uint64_t *dst = p.dst + (size_t)F::W * (coset << p.d);

    for (int li = tid; li < E; li += nt) s[li] = F::template load<A16>(src, base | ((size_t)(li >> p.c) << p.h) | (size_t)(li & cmask));
    __syncthreads();

    const int nlev = p.p_hi - p.p_lo + 1;
    for (int t = 0; t < nlev; ++t) {
        const int pbit = INV ? p.p_lo + t : p.p_hi - t;
        const int pl = pbit - p.h + p.c;
        const typename F::mem sh = bf_shift_term<F, A16>(p, coset, pbit);      // uniform over the workgroup
        const uint64_t *lt = p.ltab + (size_t)F::W * ((((size_t)1) << (p.d - 1 - pbit)) - 1);
        for (int bf = tid; bf < (E >> 1); bf += nt) {
            const int ia = ((bf >> pl) << (pl + 1)) | (bf & ((1 << pl) - 1));
            const size_t u = base | ((size_t)(ia >> p.c) << p.h) | (size_t)(ia & cmask);
            bf_apply<F, INV>(s, ia, ia | (1 << pl), F::add(F::template load<A16>(lt, u >> (pbit + 1)), sh));
        }
        __syncthreads();
    }

    for (int li = tid; li < E; li += nt) F::template store<A16>(dst, base | ((size_t)(li >> p.c) << p.h) | (size_t)(li & cmask), s[li]);
}

template<class F, bool A16> __global__ void __launch_bounds__(512, F::UPPER_WAVES) kx_bfly_upper(BfParamsX p) { bfly_upper_body<F, A16, false>(p); }
template<class F, bool A16> __global__ void __launch_bounds__(512, F::UPPER_WAVES) kx_bfly_upper_inv(BfParamsX p) { bfly_upper_body<F, A16, true>(p); }

// Forward: last pass — pair bits a_low-1 .. 0, then natural-order (bit-reversed) store.
// Inverse: first pass — natural-order load, pair bits 0 .. a_low-1, block-order store.
// natural-order side: slot sidx -> (tile g, lo, t' = rev(top)); consecutive sidx = consecutive addresses
// block-order side  : slot e    -> (tile g, top, lo)
template<class F, bool A16, bool INV>
__device__ __forceinline__ void bfly_edge_body(const BfParamsX &p)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t iopx_smem[];
    typename F::mem *s = reinterpret_cast<typename F::mem *>(iopx_smem);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int tb = p.a_low + p.c_top;                   // bits of one tile
    const int E = 1 << (tb + p.g_bits);                 // elements in LDS (2^g_bits tiles)
    const int midbits = p.d - tb;                       // tile index bits inside a coset
    const size_t unit0 = (size_t)blockIdx.x << p.g_bits;
    const int lomask = (1 << p.a_low) - 1, tmask = (1 << p.c_top) - 1;

    if (!INV) {
        for (int e = tid; e < E; e += nt) {
            const size_t unit = unit0 + (size_t)(e >> tb);
            if (unit >= p.total_units) continue;
            const size_t coset = unit >> midbits, mid = unit & (((size_t)1 << midbits) - 1);
            const int li = e & ((1 << tb) - 1), top = li >> p.a_low, lo = li & lomask;
            const size_t u = ((size_t)top << (p.d - p.c_top)) | (mid << p.a_low) | (size_t)lo;
            s[e] = F::template load<A16>(p.src, (p.src_shared ? (size_t)0 : (coset << p.d)) + u);
        }
    } else {
        for (int sidx = tid; sidx < E; sidx += nt) {
            const size_t unit = unit0 + (size_t)(sidx >> tb);
            if (unit >= p.total_units) continue;
            const size_t coset = unit >> midbits, mid = unit & (((size_t)1 << midbits) - 1);
            const int tp = sidx & tmask, lo = (sidx >> p.c_top) & lomask;
            const int top = (int)bitrev_low((uint32_t)tp, p.c_top);
            const size_t v = ((size_t)bitrev_low((uint32_t)lo, p.a_low) << (p.d - p.a_low)) |
                             ((size_t)bitrev_low((uint32_t)mid, midbits) << p.c_top) | (size_t)tp;
            s[((sidx >> tb) << tb) | (top << p.a_low) | lo] = F::template load<A16>(p.src, (coset << p.d) + v);
        }
    }
    __syncthreads();

    for (int t = 0; t < p.a_low; ++t) {
        const int pbit = INV ? t : p.a_low - 1 - t;
        const uint64_t *lt = p.ltab + (size_t)F::W * ((((size_t)1) << (p.d - 1 - pbit)) - 1);
        // one tile per workgroup: the coset, and with it the level's shift term, is uniform over the workgroup
        const typename F::mem sh0 = p.g_bits == 0 ? bf_shift_term<F, A16>(p, unit0 >> midbits, pbit) : F::zero();
        for (int bf = tid; bf < (E >> 1); bf += nt) {
            const int low = bf & ((1 << pbit) - 1), high = bf >> pbit;
            const int ia = (high << (pbit + 1)) | low, ib = ia | (1 << pbit);
            const size_t unit = unit0 + (size_t)(ia >> tb);
            if (unit >= p.total_units) continue;
            const size_t coset = unit >> midbits, mid = unit & (((size_t)1 << midbits) - 1);
            const int li = ia & ((1 << tb) - 1), top = li >> p.a_low, lo = li & lomask;
            const size_t u = ((size_t)top << (p.d - p.c_top)) | (mid << p.a_low) | (size_t)lo;
            const typename F::mem sh = p.g_bits == 0 ? sh0 : bf_shift_term<F, A16>(p, coset, pbit);
            bf_apply<F, INV>(s, ia, ib, F::add(F::template load<A16>(lt, u >> (pbit + 1)), sh));
        }
        __syncthreads();
    }

    if (!INV) {
        for (int sidx = tid; sidx < E; sidx += nt) {
            const size_t unit = unit0 + (size_t)(sidx >> tb);
            if (unit >= p.total_units) continue;
            const size_t coset = unit >> midbits, mid = unit & (((size_t)1 << midbits) - 1);
            const int tp = sidx & tmask, lo = (sidx >> p.c_top) & lomask;
            const int top = (int)bitrev_low((uint32_t)tp, p.c_top);
            const size_t v = ((size_t)bitrev_low((uint32_t)lo, p.a_low) << (p.d - p.a_low)) |
                             ((size_t)bitrev_low((uint32_t)mid, midbits) << p.c_top) | (size_t)tp;
            F::template store<A16>(p.dst, (coset << p.d) + v, s[((sidx >> tb) << tb) | (top << p.a_low) | lo]);
        }
    } else {
        for (int e = tid; e < E; e += nt) {
            const size_t unit = unit0 + (size_t)(e >> tb);
            if (unit >= p.total_units) continue;
            const size_t coset = unit >> midbits, mid = unit & (((size_t)1 << midbits) - 1);
            const int li = e & ((1 << tb) - 1), top = li >> p.a_low, lo = li & lomask;
            F::template store<A16>(p.dst, (coset << p.d) + (((size_t)top << (p.d - p.c_top)) | (mid << p.a_low) | (size_t)lo), s[e]);
        }
    }
}

template<class F, bool A16> __global__ void __launch_bounds__(512) kx_bfly_edge(BfParamsX p) { bfly_edge_body<F, A16, false>(p); }
template<class F, bool A16> __global__ void __launch_bounds__(512) kx_bfly_edge_inv(BfParamsX p) { bfly_edge_body<F, A16, true>(p); }

// ---------------------------------------------------------------------------------------------
// FRI fold (fri_aux.tcc:36-103) in the inversion-free nested form of fri_add.hip: a coset of 2^eta is folded eta times by two,
//     g[J] = f[2J] + (f[2J] + f[2J+1]) * (x + v_{2J}) / b_0 ,
// each time over the domain derived by q(X) = X^2 + b_0 X.  (x + v_{2J}) / b_0 is GF(2)-affine in the bits of J.  One launch folds up to
// three levels in registers: a lane reads its 2^ETA consecutive elements and writes one.
// ---------------------------------------------------------------------------------------------
#define FOLDX_MAX_ETA 3
struct FoldParamsX {
    const uint64_t *src;
    uint64_t *dst;
    const uint64_t *consts[FOLDX_MAX_ETA];    // level e: [0] = (x + s) / b0, [1 + k] = b_{k+1} / b0 of that level's domain
    int nbits[FOLDX_MAX_ETA];                 // number of [1 + k] entries: log2 of the level's output size
    size_t n_out;
};

template<class F, bool A16, int ETA>
__device__ __forceinline__ void fri_fold_body(const FoldParamsX &p)
{
    for (size_t C = (size_t)blockIdx.x * blockDim.x + threadIdx.x; C < p.n_out; C += (size_t)gridDim.x * blockDim.x) {
        typename F::mem v[1 << ETA];
#pragma unroll
        for (int i = 0; i < (1 << ETA); ++i) v[i] = F::template load<A16>(p.src, (C << ETA) + i);
#pragma unroll
        for (int e = 0; e < ETA; ++e) {
            const int skip = ETA - 1 - e;               // pair J = C 2^skip + q: the low `skip` index bits belong to the in-coset pair q
            typename F::mem m = F::template load<A16>(p.consts[e], 0);
            for (int k = skip; k < p.nbits[e]; ++k) if ((C >> (k - skip)) & 1) m = F::add(m, F::template load<A16>(p.consts[e], 1 + k));
#pragma unroll
            for (int q = 0; q < (1 << skip); ++q) {
                typename F::mem mq = m;
#pragma unroll
                for (int k = 0; k < skip; ++k) if ((q >> k) & 1) mq = F::add(mq, F::template load<A16>(p.consts[e], 1 + k));
                v[q] = F::add(v[2 * q], F::mul(F::add(v[2 * q], v[2 * q + 1]), mq));
            }
        }
        F::template store<A16>(p.dst, C, v[0]);
    }
}

template<class F, bool A16> __global__ void __launch_bounds__(256) kx_fri_fold1(FoldParamsX p) { fri_fold_body<F, A16, 1>(p); }
template<class F, bool A16> __global__ void __launch_bounds__(256) kx_fri_fold2(FoldParamsX p) { fri_fold_body<F, A16, 2>(p); }
template<class F, bool A16> __global__ void __launch_bounds__(256) kx_fri_fold3(FoldParamsX p) { fri_fold_body<F, A16, 3>(p); }

// ---------------------------------------------------------------------------------------------
// LDT combination (ldt_reducer_aux.tcc:39-131) over an affine subspace: x^(2^i) is GF(2)-linear, so x_j^(2^i) is a subset sum of
// basis[k]^(2^i) over the bits of j (exponentiation.tcc:3-19) and x_j^e the product over the set bits of e.  The host orders the oracles
// by their bump exponent: a lane computes x_j^e once per distinct exponent.
// ---------------------------------------------------------------------------------------------
struct LdtParamsX {
    const uint64_t *const *oracles; // device array of num_oracles device pointers, grouped by exponent
    uint64_t *out;
    const uint64_t *tab;            // [bit i][0] = shift^(2^i), [bit i][1 + k] = basis[k]^(2^i); (m + 1) elements per bit
    const uint64_t *coef;           // per oracle: c[k], then the coefficient of its shifted copy (unused when maximal)
    const uint64_t *expo;           // per oracle: max_degree - degree_k (0 = maximal), one word each
    size_t n;
    int m, num_oracles;
};

template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_ldt_combine(LdtParamsX p)
{
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < p.n; j += (size_t)gridDim.x * blockDim.x) {
        typename F::mem acc = F::zero();
        uint64_t have_e = 0;
        typename F::reg xe = F::unpack(F::one());
        for (int o = 0; o < p.num_oracles; ++o) {
            const typename F::mem f = F::template load<A16>(p.oracles[o], j);
            typename F::mem c = F::template load<A16>(p.coef, 2 * (size_t)o);
            const uint64_t e = p.expo[o];
            if (e) {
                if (e != have_e) {                      // uniform: x_j^e for this group of oracles
                    xe = F::unpack(F::one());
                    bool first = true;
                    uint64_t r = e;
                    for (int i = 0; r; ++i, r >>= 1) {
                        if (!(r & 1)) continue;
                        const size_t t = (size_t)i * (p.m + 1);
                        typename F::mem v = F::template load<A16>(p.tab, t);
                        for (int k = 0; k < p.m; ++k) if ((j >> k) & 1) v = F::add(v, F::template load<A16>(p.tab, t + 1 + k));
                        xe = first ? F::unpack(v) : F::rmul(xe, F::unpack(v));
                        first = false;
                    }
                    have_e = e;
                }
                c = F::add(c, F::pack(F::rmul(F::unpack(F::template load<A16>(p.coef, 2 * (size_t)o + 1)), xe)));
            }
            acc = F::add(acc, F::mul(c, f));
        }
        F::template store<A16>(p.out, j, acc);
    }
}

template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_mul(const uint64_t *a, const uint64_t *b, uint64_t *out, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        F::template store<A16>(out, i, F::mul(F::template load<A16>(a, i), F::template load<A16>(b, i)));
}

template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_inv(const uint64_t *a, uint64_t *out, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        F::template store<A16>(out, i, F::inv(F::template load<A16>(a, i)));
}

// ---------------------------------------------------------------------------------------------
// host: field helpers
// ---------------------------------------------------------------------------------------------
template<class H, int W>
static void push_words(std::vector<uint64_t> &v, const H &x)
{
    uint64_t w[W];
    x.store(w);
    v.insert(v.end(), w, w + W);
}

// ---------------------------------------------------------------------------------------------
// host: plans
// ---------------------------------------------------------------------------------------------
struct P1PassX { int c, h, A, j0, j1, k_start, k_end, twist_first; };
struct P2PassX { int c, h, A, p_hi, p_lo; };

template<class F>
struct AddPlanX {
    typedef typename F::host H;
    int d = 0;
    std::vector<H> betainv;                 // 1 / beta_j of recursion level j (fft.tcc:86)
    std::vector<uint64_t> sq, sq_inv;       // level j: beta_j^(2^k) (and of the inverse), d elements per level
    DevBuf ltab, pow, pow_inv;
    bool have_pow = false, have_pow_inv = false;
    std::vector<P1PassX> p1;
    std::vector<P2PassX> p2_upper;          // forward order
    int a_low = 0, c_top = 0, g_bits = 0;

    // the d recursed values of a shift (or of a coset basis vector: the recursion is GF(2)-linear), fft.tcc:94-96
    void recurse(H v, uint64_t *out) const
    {
        for (int j = 0; j < d; ++j) {
            const H ns = v * betainv[j];
            ns.store(out + F::W * j);
            v = ns.squared() + ns;
        }
    }
};

// Plans are handed out as shared_ptr: a caller keeps its plan alive while another thread's insertion evicts the cache.  A plan of dimension d
// holds EB * 2^d bytes of twiddles (EB = the element's bytes) and, once a direction has run, 2 EB * 2^d bytes of twist powers for it
// (5 EB * 2^d bytes with both: 1.25 GiB over gf64, 2.5 GiB over gf128 and 5 GiB over gf256 at d = 25); the cache is bounded by F::CACHE_BYTES of such tables
// (and 64 entries), and cleared as a whole when an insertion would pass that.
template<class F>
struct PlanCacheX {
    static std::mutex mu;
    static std::map<std::vector<uint64_t>, std::shared_ptr<AddPlanX<F>>> plans;
};
template<class F> std::mutex PlanCacheX<F>::mu;
template<class F> std::map<std::vector<uint64_t>, std::shared_ptr<AddPlanX<F>>> PlanCacheX<F>::plans;
template<class F> static size_t plan_bytes_x(const AddPlanX<F> &pl) { return pl.ltab.bytes + pl.pow.bytes + pl.pow_inv.bytes; }

template<class F>
static void clear_plans_x()
{
    std::lock_guard<std::mutex> lk(PlanCacheX<F>::mu);
    PlanCacheX<F>::plans.clear();
}

// the passes of both phases for 2^d elements in tiles of 2^tile_bits
template<class F>
static void schedule_x(AddPlanX<F> &pl, const TuningX &tu)
{
    const int d = pl.d, T = tu.tile_bits;
    // phase 1: a level whose index bits [j, d) fit one tile runs there with every level after it; a level before that takes one pass per
    // run of A - 1 network steps (a tile of 2^A rows holds the steps whose two bits lie inside it)
    const int cp = std::min(tu.p1_cols, T - 2);
    for (int j = 0; j < d; ++j) {
        if (d - j <= T) {
            const int A = d - j;
            pl.p1.push_back({ std::min(T - A, j), j, A, j, d - 1, d - 2, d - 1, 1 });
            break;
        }
        int top = d - 1, first = 1;
        for (;;) {
            const int h = std::max(j, top + 1 - (T - cp)), c = std::min(cp, h), A = top + 1 - h;
            pl.p1.push_back({ c, h, A, j, j, top - 1, h, first });
            first = 0;
            if (h == j) break;
            top = h;
        }
    }
    // phase 2: the last pass holds the low a_low pair bits (and 2^c_top natural-order runs), upper passes the rest from the top down
    if (d <= T) { pl.a_low = d; pl.c_top = 0; pl.g_bits = T - d; return; }
    pl.c_top = std::min(tu.p2_top, T - 1);
    pl.a_low = T - pl.c_top;
    pl.g_bits = 0;
    const int c = std::min(tu.p2_cols, pl.a_low), amax = T - c;
    for (int top = d - 1; top >= pl.a_low;) {
        const int h = std::max(pl.a_low, top + 1 - amax);
        pl.p2_upper.push_back({ c, h, top + 1 - h, top, h });
        top = h - 1;
    }
}

template<class F>
static int get_plan_x(const uint64_t *basis, int d, std::shared_ptr<AddPlanX<F>> *out)
{
    typedef typename F::host H;
    const size_t EB = sizeof(typename F::mem);
    const TuningX tu = tuning_x<F>();
    std::vector<uint64_t> key(basis, basis + F::W * (size_t)d);
    key.push_back((uint64_t)d);
    key.push_back((uint64_t)tu.tile_bits | ((uint64_t)tu.p1_cols << 8) | ((uint64_t)tu.p2_cols << 16) | ((uint64_t)tu.p2_top << 24));
    auto &plans = PlanCacheX<F>::plans;
    std::lock_guard<std::mutex> lk(PlanCacheX<F>::mu);
    auto it = plans.find(key);
    if (it != plans.end()) { *out = it->second; return IOPX_OK; }
    size_t resident = EB << d;
    for (const auto &kv : plans) resident += plan_bytes_x(*kv.second);
    if (plans.size() >= 64 || resident > F::CACHE_BYTES) { (void)hipStreamSynchronize(stream()); plans.clear(); }
    ColdScope cs_(F::cold_plan());
    std::shared_ptr<AddPlanX<F>> pl(new AddPlanX<F>);
    pl->d = d;
    std::vector<H> b2(d);
    for (int i = 0; i < d; ++i) b2[i] = H(basis + F::W * i);
    std::vector<uint64_t> rec;                      // recursed basis vectors, level j has d-1-j
    for (int j = 0; j < d; ++j) {
        const H beta = b2[d - 1 - j];
        if (beta.is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "additive FFT: basis vectors are linearly dependent");
        const H binv = beta.inverse();
        pl->betainv.push_back(binv);
        H s = beta, si = binv;
        for (int k = 0; k < d; ++k) { push_words<H, F::W>(pl->sq, s); push_words<H, F::W>(pl->sq_inv, si); s = s.squared(); si = si.squared(); }
        for (int i = 0; i < d - 1 - j; ++i) {
            const H nb = b2[i] * binv;
            push_words<H, F::W>(rec, nb);
            b2[i] = nb.squared() + nb;
        }
    }
    schedule_x(*pl, tu);
    int rc = pl->ltab.alloc(EB << d);
    if (rc != IOPX_OK) return rc;
    if (d > 1) {
        TmpBuf drec;
        if ((rc = drec.alloc(rec.size() * 8)) != IOPX_OK) return rc;
        if ((rc = upload(drec.p, rec.data(), rec.size() * 8)) != IOPX_OK) return rc;
        const size_t count = ((size_t)1 << d) - 1;
        IOPX_LAUNCHX(al16(pl->ltab.p) && al16(drec.p), "build_ltab", 0, kx_build_ltab, dim3(grid_x(count, 256)), dim3(256), 0,
                     pl->ltab.u64(), drec.u64(), d, count);
        IOPX_HIP(hipGetLastError());
    } else {
        if ((rc = fill_bytes(pl->ltab.p, 0, 2 * EB)) != IOPX_OK) return rc;
    }
    *out = pl;
    plans[key] = std::move(pl);
    return IOPX_OK;
}

// twist-power tables of one direction, built on first use
template<class F>
static int ensure_pow_x(AddPlanX<F> &pl, bool inverse)
{
    const size_t EB = sizeof(typename F::mem);
    std::lock_guard<std::mutex> lk(PlanCacheX<F>::mu);      // the tables of a shared plan are built once
    if (inverse ? pl.have_pow_inv : pl.have_pow) return IOPX_OK;
    ColdScope cs_(F::cold_pow());
    DevBuf &buf = inverse ? pl.pow_inv : pl.pow;
    const std::vector<uint64_t> &sq = inverse ? pl.sq_inv : pl.sq;
    const int d = pl.d;
    int rc = buf.alloc((2 * EB) << d);
    if (rc != IOPX_OK) return rc;
    TmpBuf dsq;
    if ((rc = dsq.alloc(sq.size() * 8)) != IOPX_OK) return rc;
    if ((rc = upload(dsq.p, sq.data(), sq.size() * 8)) != IOPX_OK) return rc;
    const bool a16 = al16(buf.p) && al16(dsq.p);
    for (int j = 0; j < d; ++j) {
        const size_t off = (((size_t)2) << d) - (((size_t)2) << (d - j)), count = (size_t)1 << (d - j);
        IOPX_LAUNCHX(a16, "pow_direct", 0, kx_pow_direct, dim3(grid_x(count, 256)), dim3(256), 0, buf.u64() + F::W * off,
                     dsq.u64() + F::W * (size_t)j * d, d - j, count);
    }
    IOPX_HIP(hipGetLastError());
    (inverse ? pl.have_pow_inv : pl.have_pow) = true;
    return IOPX_OK;
}

template<class F, bool INV>
static int run_phase1_x(AddPlanX<F> &pl, uint64_t *S)
{
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_pow_x(pl, INV);
    if (rc != IOPX_OK) return rc;
    const size_t np = pl.p1.size();
    const bool a16 = al16(S) && al16((INV ? pl.pow_inv : pl.pow).p);
    for (size_t i = 0; i < np; ++i) {
        const P1PassX &ps = pl.p1[INV ? np - 1 - i : i];
        P1ParamsX p;
        p.S = S; p.pow = (INV ? pl.pow_inv : pl.pow).u64(); p.d = pl.d;
        p.c = ps.c; p.h = ps.h; p.A = ps.A; p.j0 = ps.j0; p.j1 = ps.j1; p.k_start = ps.k_start; p.k_end = ps.k_end; p.twist_first = ps.twist_first;
        const int tb = ps.c + ps.A;
        const size_t E = (size_t)1 << tb, grid = (size_t)1 << (pl.d - tb);
        const int threads = (int)std::min<size_t>(512, std::max<size_t>(64, E / 4));
        if (INV) IOPX_LAUNCHX(a16, "phase1_inv", (2 * EB) << pl.d, kx_phase1_inv, dim3((unsigned)grid), dim3(threads), E * EB, p);
        else IOPX_LAUNCHX(a16, "phase1", (2 * EB) << pl.d, kx_phase1, dim3((unsigned)grid), dim3(threads), E * EB, p);
    }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

// rs[v * d + p] for the shift (v = 0) and the nhi coset basis vectors, on the device
template<class F>
static int upload_rs_x(const AddPlanX<F> &pl, const uint64_t *shift, const uint64_t *hi_basis, int nhi, TmpBuf &drs)
{
    typedef typename F::host H;
    std::vector<uint64_t> rs((size_t)(1 + nhi) * pl.d * F::W);
    pl.recurse(H(shift), rs.data());
    for (int v = 0; v < nhi; ++v) pl.recurse(H(hi_basis + F::W * v), rs.data() + (size_t)(1 + v) * pl.d * F::W);
    int rc = drs.alloc(rs.size() * 8);
    if (rc != IOPX_OK) return rc;
    return upload(drs.p, rs.data(), rs.size() * 8);
}

template<class F>
static BfParamsX bf_params_x(const AddPlanX<F> &pl, const uint64_t *rs, int nhi)
{
    BfParamsX p;
    memset(&p, 0, sizeof(p));
    p.ltab = pl.ltab.u64(); p.rs = rs; p.d = pl.d; p.nhi = nhi;
    p.a_low = pl.a_low; p.c_top = pl.c_top; p.g_bits = pl.g_bits;
    return p;
}

static bool bf_a16(const BfParamsX &p) { return al16(p.src) && al16(p.dst) && al16(p.rs) && al16(p.ltab); }

template<class F>
static void launch_upper_x(bool inv, BfParamsX p, const P2PassX &ps, size_t cosets, bool batch = false)
{
    const size_t EB = sizeof(typename F::mem);
    p.c = ps.c; p.h = ps.h; p.A = ps.A; p.p_hi = ps.p_hi; p.p_lo = ps.p_lo;
    const int tb = ps.c + ps.A;
    const size_t E = (size_t)1 << tb, grid = cosets << (p.d - tb);
    const int threads = (int)std::min<size_t>(512, std::max<size_t>(64, E / 2));
    if (inv) IOPX_LAUNCHX(bf_a16(p), batch ? "bfly_upper_inv_batch" : "bfly_upper_inv", (cosets * 2 * EB) << p.d, kx_bfly_upper_inv, dim3((unsigned)grid), dim3(threads), E * EB, p);
    else IOPX_LAUNCHX(bf_a16(p), "bfly_upper", (cosets * 2 * EB) << p.d, kx_bfly_upper, dim3((unsigned)grid), dim3(threads), E * EB, p);
}

template<class F>
static void launch_edge_x(bool inv, BfParamsX p, size_t cosets, bool batch = false)
{
    const size_t EB = sizeof(typename F::mem);
    const int tb = p.a_low + p.c_top;
    p.total_units = cosets << (p.d - tb);
    const size_t E = (size_t)1 << (tb + p.g_bits), grid = (p.total_units + (((size_t)1) << p.g_bits) - 1) >> p.g_bits;
    const int threads = (int)std::min<size_t>(512, std::max<size_t>(64, E / 2));
    if (inv) IOPX_LAUNCHX(bf_a16(p), batch ? "bfly_edge_inv_batch" : "bfly_edge_inv", (cosets * 2 * EB) << p.d, kx_bfly_edge_inv, dim3((unsigned)grid), dim3(threads), E * EB, p);
    else IOPX_LAUNCHX(bf_a16(p), "bfly_edge", (cosets * 2 * EB) << p.d, kx_bfly_edge, dim3((unsigned)grid), dim3(threads), E * EB, p);
}

// forward phase 2 of cosets [coset_begin, +coset_count): W (2^d, block order after phase 1, overwritten when it is the only coset) -> out
template<class F>
static int run_phase2_fwd_x(AddPlanX<F> &pl, uint64_t *W, uint64_t *out, const uint64_t *rs, int nhi, size_t coset_begin, size_t coset_count)
{
    const size_t EB = sizeof(typename F::mem);
    const int d = pl.d;
    BfParamsX p = bf_params_x(pl, rs, nhi);
    if (pl.p2_upper.empty()) {                      // one tile per coset: W -> out in one pass
        // the unit count of a launch stays below 2^31 workgroups
        const size_t step = (size_t)1 << 30;
        for (size_t c0 = 0; c0 < coset_count; c0 += step) {
            const size_t cnt = std::min(step, coset_count - c0);
            p.src = W; p.src_shared = 1; p.dst = out + F::W * (c0 << d); p.coset_base = coset_begin + c0;
            launch_edge_x<F>(false, p, cnt);
        }
        IOPX_HIP(hipGetLastError());
        return IOPX_OK;
    }
    if (coset_count == 1) {
        p.src = W; p.dst = W; p.src_shared = 0; p.coset_base = coset_begin;
        for (const P2PassX &ps : pl.p2_upper) launch_upper_x<F>(false, p, ps, 1);
        p.dst = out;
        launch_edge_x<F>(false, p, 1);
        IOPX_HIP(hipGetLastError());
        return IOPX_OK;
    }
    // block-order staging for a group of cosets (the last pass permutes: it cannot run in place), at most 2^STAGE_BITS elements
    const size_t group = std::min(coset_count, std::max<size_t>(1, ((size_t)1 << F::STAGE_BITS) >> d));
    TmpBuf stage;
    int rc = stage.alloc((group * EB) << d);
    if (rc != IOPX_OK) return rc;
    for (size_t c0 = 0; c0 < coset_count; c0 += group) {
        const size_t cnt = std::min(group, coset_count - c0);
        p.coset_base = coset_begin + c0;
        p.dst = stage.u64();
        for (size_t i = 0; i < pl.p2_upper.size(); ++i) {
            p.src = i == 0 ? W : stage.u64(); p.src_shared = i == 0;
            launch_upper_x<F>(false, p, pl.p2_upper[i], cnt);
        }
        p.src = stage.u64(); p.src_shared = 0; p.dst = out + F::W * (c0 << d);
        launch_edge_x<F>(false, p, cnt);
    }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

static int check_basis_args_x(const uint64_t *basis, size_t m, const uint64_t *shift)
{
    if (m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension %zu too large", m);
    if ((m > 0 && !basis) || !shift) return fail(IOPX_ERR_INVALID_ARGUMENT, "null basis/shift");
    return IOPX_OK;
}

// ---------------------------------------------------------------------------------------------
// the bodies of the C entries (iopx_*_gf64*, iopx_*_gf128*, iopx_*_gf256*)
// ---------------------------------------------------------------------------------------------
// Cosets [coset_begin, coset_begin + coset_count) of span(basis[0..d)), d = ceil(log2 n_coeffs): the
// contiguous output block [coset_begin * 2^d, (coset_begin + coset_count) * 2^d) of the full transform.
template<class F>
static int x_add_lde_dev(const uint64_t *d_coeffs, size_t n_coeffs, const uint64_t *basis, size_t m,
                         const uint64_t *shift, size_t coset_begin, size_t coset_count, uint64_t *d_out)
{
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    rc = check_basis_args_x(basis, m, shift);
    if (rc != IOPX_OK) return rc;
    const size_t n = (size_t)1 << m;
    if (n_coeffs > n) return fail(IOPX_ERR_INVALID_ARGUMENT, "additive FFT: %zu coefficients exceed the domain size %zu", n_coeffs, n);
    if (!d_out || (n_coeffs && !d_coeffs)) return fail(IOPX_ERR_INVALID_ARGUMENT, "null buffer");
    const int d = n_coeffs <= 1 ? 0 : (int)ceil_log2(n_coeffs);
    const int nhi = (int)m - d;
    const size_t all_cosets = (size_t)1 << nhi;
    if (coset_count == 0 || coset_begin >= all_cosets || coset_count > all_cosets - coset_begin)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "coset range [%zu, +%zu) outside the %zu cosets of the transform", coset_begin, coset_count, all_cosets);
    if (n_coeffs <= 1) {
        IOPX_LAUNCHX(al16(d_out) && al16(d_coeffs), "fill", 0, kx_fill, dim3(grid_x(coset_count, 256)), dim3(256), 0, d_out, d_coeffs,
                     (int)(n_coeffs == 1), coset_count);
        IOPX_HIP(hipGetLastError());
        return IOPX_OK;
    }
    std::shared_ptr<AddPlanX<F>> pl;
    rc = get_plan_x<F>(basis, d, &pl);
    if (rc != IOPX_OK) return rc;
    TmpBuf drs;
    rc = upload_rs_x(*pl, shift, basis + F::W * (size_t)d, nhi, drs);
    if (rc != IOPX_OK) return rc;

    // phase 1 runs in a work buffer: the last pass permutes into natural order and therefore writes out of place
    const size_t nd = (size_t)1 << d;
    TmpBuf work;
    rc = work.alloc(nd * EB);
    if (rc != IOPX_OK) return rc;
    uint64_t *W = work.u64();
    IOPX_LAUNCHX(al16(W) && al16(d_coeffs), "pad_copy", 0, kx_pad_copy, dim3(grid_x(nd, 256)), dim3(256), 0, W, d_coeffs, n_coeffs, nd);
    rc = run_phase1_x<F, false>(*pl, W);
    if (rc != IOPX_OK) return rc;
    return run_phase2_fwd_x(*pl, W, d_out, drs.u64(), nhi, coset_begin, coset_count);      // temporaries are released in stream order
}

template<class F>
static int x_add_fft_dev(const uint64_t *d_coeffs, size_t n_coeffs, const uint64_t *basis, size_t m,
                         const uint64_t *shift, uint64_t *d_out)
{
    if (m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension %zu too large", m);
    const size_t n = (size_t)1 << m;
    if (n_coeffs > n) return fail(IOPX_ERR_INVALID_ARGUMENT, "additive FFT: %zu coefficients exceed the domain size %zu", n_coeffs, n);
    const int d = n_coeffs <= 1 ? 0 : (int)ceil_log2(n_coeffs);
    return x_add_lde_dev<F>(d_coeffs, n_coeffs, basis, m, shift, 0, (size_t)1 << ((int)m - d), d_out);
}

template<class F>
static int x_add_ifft_dev(const uint64_t *d_evals, const uint64_t *basis, size_t m, const uint64_t *shift,
                          uint64_t *d_out)
{
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    rc = check_basis_args_x(basis, m, shift);
    if (rc != IOPX_OK) return rc;
    if (!d_evals || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null buffer");
    if (m == 0) return copy_d2d(d_out, d_evals, EB);
    std::shared_ptr<AddPlanX<F>> pl;
    rc = get_plan_x<F>(basis, (int)m, &pl);
    if (rc != IOPX_OK) return rc;
    TmpBuf drs;
    rc = upload_rs_x(*pl, shift, nullptr, 0, drs);
    if (rc != IOPX_OK) return rc;
    // the first pass permutes: in place, the transform runs in a work buffer and is copied back
    TmpBuf work;
    uint64_t *W = d_out;
    if (d_evals == d_out) {
        rc = work.alloc(EB << m);
        if (rc != IOPX_OK) return rc;
        W = work.u64();
    }
    BfParamsX p = bf_params_x(*pl, drs.u64(), 0);
    p.src = d_evals; p.dst = W;
    launch_edge_x<F>(true, p, 1);
    p.src = W;
    for (size_t i = pl->p2_upper.size(); i-- > 0;) launch_upper_x<F>(true, p, pl->p2_upper[i], 1);
    IOPX_HIP(hipGetLastError());
    rc = run_phase1_x<F, true>(*pl, W);
    if (rc != IOPX_OK) return rc;
    if (W != d_out) return copy_d2d(d_out, W, EB << m);
    return IOPX_OK;
}

// ---------------------------------------------------------------------------------------------
// batched forms: several vectors over ONE domain share every launch (x_add_ifft_batch_dev, x_add_lde_batch_dev), and the fused re-extension
// (x_add_reextend_lde_batch_dev).  The kernels are the bodies above under a second grid dimension: workgroup (x, v) does for vector v what
// workgroup x does in the single-vector launch, so the outputs are the single-vector entries' bit for bit.  An inverse pass over `batch` vectors
// stored back to back needs no second dimension: with no coset basis (nhi = 0) the vectors are the "cosets" of the single-vector kernels, and
// 2^g_bits small vectors share one workgroup's tile as cosets do.  The profile reports every launch of this section under the kernel's name + "_batch".
// ---------------------------------------------------------------------------------------------
struct BfBatchParamsX {
    BfParamsX p;                    // src / dst: vector 0's
    const uint64_t *const *dsts;    // last pass: device array of the vectors' outputs (the caller's d_outs)
    size_t src_stride, dst_stride;  // elements from one vector to the next in src / in dst (upper passes)
    size_t dst_off;                 // last pass: elements added to dsts[v] (the coset group's offset)
};

template<class F, bool A16>
__global__ void __launch_bounds__(512, F::UPPER_WAVES) kx_bfly_upper_batch(BfBatchParamsX q)
{
    BfParamsX p = q.p;
    p.src += (size_t)F::W * blockIdx.y * q.src_stride;
    p.dst += (size_t)F::W * blockIdx.y * q.dst_stride;
    bfly_upper_body<F, A16, false>(p);
}

template<class F, bool A16>
__global__ void __launch_bounds__(512) kx_bfly_edge_batch(BfBatchParamsX q)
{
    BfParamsX p = q.p;
    p.src += (size_t)F::W * blockIdx.y * q.src_stride;
    p.dst = const_cast<uint64_t *>(q.dsts[blockIdx.y]) + (size_t)F::W * q.dst_off;
    bfly_edge_body<F, A16, false>(p);
}

struct P1BatchParamsX { P1ParamsX p; size_t stride; };
template<class F, bool A16> __global__ void __launch_bounds__(512) kx_phase1_batch(P1BatchParamsX q)
{
    P1ParamsX p = q.p;
    p.S += (size_t)F::W * blockIdx.y * q.stride;
    phase1_body<F, A16, false>(p);
}
template<class F, bool A16> __global__ void __launch_bounds__(512) kx_phase1_inv_batch(P1BatchParamsX q)
{
    P1ParamsX p = q.p;
    p.S += (size_t)F::W * blockIdx.y * q.stride;
    phase1_body<F, A16, true>(p);
}

// dst + v * 2^d <- srcs[v] zero padded, for every vector v of the grid's second dimension
template<class F, bool A16>
__global__ void __launch_bounds__(256) kx_pad_copy_batch(uint64_t *dst, const uint64_t *const *srcs, size_t n_src, size_t n_dst)
{
    const uint64_t *src = srcs[blockIdx.y];
    uint64_t *out = dst + (size_t)F::W * blockIdx.y * n_dst;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_dst; i += (size_t)gridDim.x * blockDim.x)
        F::template store<A16>(out, i, i < n_src ? F::template load<A16>(src, i) : F::zero());
}

static const size_t BATCH_MAX_X = 65535;           // the second grid dimension's bound

// phase 1 of `count` vectors of 2^d elements back to back at S: one launch per pass
template<class F, bool INV>
static int run_phase1_batch_x(AddPlanX<F> &pl, uint64_t *S, size_t count)
{
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_pow_x(pl, INV);
    if (rc != IOPX_OK) return rc;
    const size_t np = pl.p1.size();
    const bool a16 = al16(S) && al16((INV ? pl.pow_inv : pl.pow).p);      // an element is 16 bytes or more where it matters: every vector is aligned as the first
    for (size_t i = 0; i < np; ++i) {
        const P1PassX &ps = pl.p1[INV ? np - 1 - i : i];
        P1BatchParamsX q;
        P1ParamsX &p = q.p;
        p.S = S; p.pow = (INV ? pl.pow_inv : pl.pow).u64(); p.d = pl.d;
        p.c = ps.c; p.h = ps.h; p.A = ps.A; p.j0 = ps.j0; p.j1 = ps.j1; p.k_start = ps.k_start; p.k_end = ps.k_end; p.twist_first = ps.twist_first;
        q.stride = (size_t)1 << pl.d;
        const int tb = ps.c + ps.A;
        const size_t E = (size_t)1 << tb, grid = (size_t)1 << (pl.d - tb);
        const int threads = (int)std::min<size_t>(512, std::max<size_t>(64, E / 4));
        if (INV) IOPX_LAUNCHX(a16, "phase1_inv_batch", (count * 2 * EB) << pl.d, kx_phase1_inv_batch, dim3((unsigned)grid, (unsigned)count), dim3(threads), E * EB, q);
        else IOPX_LAUNCHX(a16, "phase1_batch", (count * 2 * EB) << pl.d, kx_phase1_batch, dim3((unsigned)grid, (unsigned)count), dim3(threads), E * EB, q);
    }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

// inverse phase 2 of `count` vectors back to back (natural order at src -> block order at dst, src != dst): the vectors as the cosets of the
// single-vector kernels, rs = the recursed shift alone
template<class F>
static int run_phase2_inv_batch_x(AddPlanX<F> &pl, const uint64_t *src, uint64_t *dst, const uint64_t *rs, size_t count)
{
    BfParamsX p = bf_params_x(pl, rs, 0);
    p.src = src; p.dst = dst;
    launch_edge_x<F>(true, p, count, true);
    p.src = dst;
    for (size_t i = pl.p2_upper.size(); i-- > 0;) launch_upper_x<F>(true, p, pl.p2_upper[i], count, true);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static void launch_upper_batch_x(BfBatchParamsX q, const P2PassX &ps, size_t cosets, size_t vectors, bool a16)
{
    const size_t EB = sizeof(typename F::mem);
    BfParamsX &p = q.p;
    p.c = ps.c; p.h = ps.h; p.A = ps.A; p.p_hi = ps.p_hi; p.p_lo = ps.p_lo;
    const int tb = ps.c + ps.A;
    const size_t E = (size_t)1 << tb, grid = cosets << (p.d - tb);
    const int threads = (int)std::min<size_t>(512, std::max<size_t>(64, E / 2));
    IOPX_LAUNCHX(a16, "bfly_upper_batch", (vectors * cosets * 2 * EB) << p.d, kx_bfly_upper_batch, dim3((unsigned)grid, (unsigned)vectors), dim3(threads), E * EB, q);
}

template<class F>
static void launch_edge_batch_x(BfBatchParamsX q, size_t cosets, size_t vectors, bool a16)
{
    const size_t EB = sizeof(typename F::mem);
    BfParamsX &p = q.p;
    const int tb = p.a_low + p.c_top;
    p.total_units = cosets << (p.d - tb);
    const size_t E = (size_t)1 << (tb + p.g_bits), grid = (p.total_units + (((size_t)1) << p.g_bits) - 1) >> p.g_bits;
    const int threads = (int)std::min<size_t>(512, std::max<size_t>(64, E / 2));
    IOPX_LAUNCHX(a16, "bfly_edge_batch", (vectors * cosets * 2 * EB) << p.d, kx_bfly_edge_batch, dim3((unsigned)grid, (unsigned)vectors), dim3(threads), E * EB, q);
}

// Forward phase 2 of cosets [coset_begin, +coset_count) for `total` vectors of 2^d elements in block order, back to back at Wk (overwritten), into the
// outputs d_dsts[v] (a device array; outs_a16: every one of them is 16-byte aligned).  The block-order staging of the upper passes holds a
// group of cosets of a group of vectors, at most 2^STAGE_BITS elements as in run_phase2_fwd_x (one coset of one vector where that is
// already more): a batch that does not fit takes the coset range, and then the vectors, in several rounds.
template<class F>
static int run_phase2_fwd_batch_x(AddPlanX<F> &pl, uint64_t *Wk, size_t total, const uint64_t *const *d_dsts, bool outs_a16, const uint64_t *rs, int nhi,
                                  size_t coset_begin, size_t coset_count)
{
    const size_t EB = sizeof(typename F::mem);
    const int d = pl.d;
    const size_t nd = (size_t)1 << d;
    BfBatchParamsX q;
    memset(&q, 0, sizeof(q));
    q.p = bf_params_x(pl, rs, nhi);
    BfParamsX &p = q.p;
    const bool a16 = al16(Wk) && al16(rs) && al16(p.ltab);
    if (pl.p2_upper.empty() || coset_count == 1) {          // no staging: one pass from Wk, or the upper passes in place on Wk
        for (size_t v0 = 0; v0 < total; v0 += BATCH_MAX_X) {
            const size_t nv = std::min(BATCH_MAX_X, total - v0);
            p.src = Wk + F::W * v0 * nd; p.dst = Wk + F::W * v0 * nd;
            q.src_stride = nd; q.dst_stride = nd; q.dsts = d_dsts + v0;
            if (pl.p2_upper.empty()) {
                const size_t step = (size_t)1 << 30;        // the unit count of a launch stays below 2^31 workgroups
                for (size_t c0 = 0; c0 < coset_count; c0 += step) {
                    p.src_shared = 1; p.coset_base = coset_begin + c0; q.dst_off = c0 << d;
                    launch_edge_batch_x<F>(q, std::min(step, coset_count - c0), nv, a16 && outs_a16);
                }
            } else {
                p.src_shared = 0; p.coset_base = coset_begin; q.dst_off = 0;
                for (const P2PassX &ps : pl.p2_upper) launch_upper_batch_x<F>(q, ps, 1, nv, a16);
                launch_edge_batch_x<F>(q, 1, nv, a16 && outs_a16);
            }
        }
        IOPX_HIP(hipGetLastError());
        return IOPX_OK;
    }
    const int stage_bits = opt_range("IOPX_GFX_BATCH_STAGE_BITS", F::STAGE_BITS, 0, F::STAGE_BITS);       // the tests lower it to reach the rounds at small sizes
    const size_t slots = std::max<size_t>(1, ((size_t)1 << stage_bits) >> d);                               // cosets of single vectors the staging may hold
    const size_t nvmax = std::min(std::min(total, slots), BATCH_MAX_X), group = std::min(coset_count, std::max<size_t>(1, slots / nvmax));
    TmpBuf stage;
    int rc = stage.alloc((nvmax * group * EB) << d);
    if (rc != IOPX_OK) return rc;
    const bool sa16 = a16 && al16(stage.p);
    for (size_t v0 = 0; v0 < total; v0 += nvmax) {
        const size_t nv = std::min(nvmax, total - v0);
        for (size_t c0 = 0; c0 < coset_count; c0 += group) {
            const size_t cnt = std::min(group, coset_count - c0);
            p.coset_base = coset_begin + c0;
            p.dst = stage.u64(); q.dst_stride = group << d;
            for (size_t i = 0; i < pl.p2_upper.size(); ++i) {
                if (i == 0) { p.src = Wk + F::W * v0 * nd; p.src_shared = 1; q.src_stride = nd; }
                else { p.src = stage.u64(); p.src_shared = 0; q.src_stride = group << d; }
                launch_upper_batch_x<F>(q, pl.p2_upper[i], cnt, nv, sa16);
            }
            p.src = stage.u64(); p.src_shared = 0; q.src_stride = group << d;
            q.dsts = d_dsts + v0; q.dst_off = c0 << d;
            launch_edge_batch_x<F>(q, cnt, nv, sa16 && outs_a16);
        }
    }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

// the recursed shift terms of H's shift alone and of L's shift with its coset basis, in one table: rs_H at element 0, rs_L at element d
template<class F>
static int upload_rs2_x(const AddPlanX<F> &pl, const uint64_t *eval_shift, const uint64_t *shift, const uint64_t *hi_basis, int nhi, TmpBuf &drs)
{
    typedef typename F::host H;
    std::vector<uint64_t> rs((size_t)(2 + nhi) * pl.d * F::W);
    pl.recurse(H(eval_shift), rs.data());
    pl.recurse(H(shift), rs.data() + (size_t)pl.d * F::W);
    for (int v = 0; v < nhi; ++v) pl.recurse(H(hi_basis + F::W * v), rs.data() + (size_t)(2 + v) * pl.d * F::W);
    int rc = drs.alloc(rs.size() * 8);
    if (rc != IOPX_OK) return rc;
    return upload(drs.p, rs.data(), rs.size() * 8);
}

// a host array of device pointers on the device; *a16: every one of them is 16-byte aligned
static int upload_ptrs_x(const uint64_t *const *a, size_t na, const uint64_t *const *b, size_t nb, TmpBuf &dptrs, bool *a16)
{
    std::vector<uint64_t> h;
    *a16 = true;
    for (size_t k = 0; k < na; ++k) { h.push_back((uint64_t)(uintptr_t)a[k]); *a16 = *a16 && al16(a[k]); }
    for (size_t k = 0; k < nb; ++k) { h.push_back((uint64_t)(uintptr_t)b[k]); *a16 = *a16 && al16(b[k]); }
    int rc = dptrs.alloc(h.size() * 8);
    if (rc != IOPX_OK) return rc;
    return upload(dptrs.p, h.data(), h.size() * 8);
}

static int check_batch_x(size_t batch)
{
    if (batch == 0 || batch > 65535) return fail(IOPX_ERR_INVALID_ARGUMENT, "batch size %zu outside 1..65535", batch);
    return IOPX_OK;
}

// `batch` inverse transforms over the same domain, vectors stored back to back (d_evals and d_out: batch * 2^m elements)
template<class F>
static int x_add_ifft_batch_dev(const uint64_t *d_evals, size_t batch, const uint64_t *basis, size_t m, const uint64_t *shift, uint64_t *d_out)
{
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    rc = check_basis_args_x(basis, m, shift);
    if (rc != IOPX_OK) return rc;
    if (!d_evals || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null buffer");
    if ((rc = check_batch_x(batch)) != IOPX_OK) return rc;
    const size_t bytes = (batch * EB) << m;
    if (m == 0) return copy_d2d(d_out, d_evals, bytes);
    std::shared_ptr<AddPlanX<F>> pl;
    rc = get_plan_x<F>(basis, (int)m, &pl);
    if (rc != IOPX_OK) return rc;
    TmpBuf drs;
    rc = upload_rs_x(*pl, shift, nullptr, 0, drs);
    if (rc != IOPX_OK) return rc;
    // the first pass permutes: in place, the transforms run in a work buffer and are copied back
    TmpBuf work;
    uint64_t *W = d_out;
    if (d_evals == d_out) {
        rc = work.alloc(bytes);
        if (rc != IOPX_OK) return rc;
        W = work.u64();
    }
    rc = run_phase2_inv_batch_x(*pl, d_evals, W, drs.u64(), batch);
    if (rc != IOPX_OK) return rc;
    rc = run_phase1_batch_x<F, true>(*pl, W, batch);
    if (rc != IOPX_OK) return rc;
    if (W != d_out) return copy_d2d(d_out, W, bytes);
    return IOPX_OK;
}

// `batch` low-degree extensions over the same domain: polynomial k (n_coeffs coefficients at d_coeffs[k]) -> cosets [coset_begin, +coset_count)
// of its transform at d_outs[k]
template<class F>
static int x_add_lde_batch_dev(const uint64_t *const *d_coeffs, size_t n_coeffs, size_t batch, const uint64_t *basis, size_t m, const uint64_t *shift,
                               size_t coset_begin, size_t coset_count, uint64_t *const *d_outs)
{
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    rc = check_basis_args_x(basis, m, shift);
    if (rc != IOPX_OK) return rc;
    if (!d_coeffs || !d_outs) return fail(IOPX_ERR_INVALID_ARGUMENT, "null buffer");
    if ((rc = check_batch_x(batch)) != IOPX_OK) return rc;
    for (size_t k = 0; k < batch; ++k) if (!d_coeffs[k] || !d_outs[k]) return fail(IOPX_ERR_INVALID_ARGUMENT, "null buffer");
    const size_t n = (size_t)1 << m;
    if (n_coeffs > n) return fail(IOPX_ERR_INVALID_ARGUMENT, "additive FFT: %zu coefficients exceed the domain size %zu", n_coeffs, n);
    if (n_coeffs <= 1) {                                    // constants: one fill each
        for (size_t k = 0; k < batch; ++k) {
            rc = x_add_lde_dev<F>(d_coeffs[k], n_coeffs, basis, m, shift, coset_begin, coset_count, d_outs[k]);
            if (rc != IOPX_OK) return rc;
        }
        return IOPX_OK;
    }
    const int d = (int)ceil_log2(n_coeffs);
    const int nhi = (int)m - d;
    const size_t all_cosets = (size_t)1 << nhi, nd = (size_t)1 << d;
    if (coset_count == 0 || coset_begin >= all_cosets || coset_count > all_cosets - coset_begin)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "coset range [%zu, +%zu) outside the %zu cosets of the transform", coset_begin, coset_count, all_cosets);
    std::shared_ptr<AddPlanX<F>> pl;
    rc = get_plan_x<F>(basis, d, &pl);
    if (rc != IOPX_OK) return rc;
    TmpBuf drs, dptrs, work;
    rc = upload_rs_x(*pl, shift, basis + F::W * (size_t)d, nhi, drs);
    if (rc != IOPX_OK) return rc;
    bool ptrs_a16;
    rc = upload_ptrs_x(d_outs, batch, d_coeffs, batch, dptrs, &ptrs_a16);
    if (rc != IOPX_OK) return rc;
    rc = work.alloc(batch * nd * EB);
    if (rc != IOPX_OK) return rc;
    const uint64_t *const *dev_outs = (const uint64_t *const *)dptrs.u64();
    IOPX_LAUNCHX(al16(work.p) && ptrs_a16, "pad_copy_batch", 0, kx_pad_copy_batch, dim3(grid_x(nd, 256), (unsigned)batch), dim3(256), 0, work.u64(), dev_outs + batch,
                 n_coeffs, nd);
    rc = run_phase1_batch_x<F, false>(*pl, work.u64(), batch);
    if (rc != IOPX_OK) return rc;
    return run_phase2_fwd_batch_x(*pl, work.u64(), batch, dev_outs, ptrs_a16, drs.u64(), nhi, coset_begin, coset_count);
}

// FFT_over_field_subset(IFFT_over_field_subset(evals, H), L) for `batch` vectors back to back, H = span(basis[0..d_dim)) + eval_shift and
// L = span(basis[0..m)) + shift, together with the codewords of n_polys polynomials of n_coeffs <= 2^d_dim coefficients (d_outs: the re-extensions,
// then the codewords).  Phase 1 depends on the basis prefix only, not on the shift, so the inverse transform's last half and the forward transform's
// first half cancel exactly: H's butterflies are undone into block order and the butterflies of L's cosets applied to that, with no phase-1 pass and no
// coefficient vector in between; the polynomials join after a phase 1 of their own, and every forward launch serves both kinds.
template<class F>
static int x_add_reextend_lde_batch_dev(const uint64_t *d_evals, size_t batch, const uint64_t *const *d_coeffs, size_t n_coeffs, size_t n_polys,
                                        const uint64_t *basis, size_t m, size_t d_dim, const uint64_t *eval_shift, const uint64_t *shift,
                                        size_t coset_begin, size_t coset_count, uint64_t *const *d_outs)
{
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    rc = check_basis_args_x(basis, m, shift);
    if (rc != IOPX_OK) return rc;
    if (!d_evals || !d_outs || !eval_shift || (n_polys && !d_coeffs)) return fail(IOPX_ERR_INVALID_ARGUMENT, "null buffer");
    if (batch == 0 || batch > 65535 || n_polys > 65535) return fail(IOPX_ERR_INVALID_ARGUMENT, "batch size %zu + %zu outside 1..65535", batch, n_polys);
    if (d_dim > m) return fail(IOPX_ERR_INVALID_ARGUMENT, "the evaluation domain must be spanned by the first basis vectors of the codeword domain");
    for (size_t k = 0; k < batch + n_polys; ++k) if (!d_outs[k]) return fail(IOPX_ERR_INVALID_ARGUMENT, "null buffer");
    for (size_t k = 0; k < n_polys; ++k) if (!d_coeffs[k]) return fail(IOPX_ERR_INVALID_ARGUMENT, "null buffer");
    const int d = (int)d_dim, nhi = (int)m - d;
    const size_t all_cosets = (size_t)1 << nhi, nd = (size_t)1 << d;
    if (n_polys && n_coeffs > nd) return fail(IOPX_ERR_INVALID_ARGUMENT, "%zu coefficients exceed the 2^%d of the evaluation domain", n_coeffs, d);
    if (coset_count == 0 || coset_begin >= all_cosets || coset_count > all_cosets - coset_begin)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "coset range [%zu, +%zu) outside the %zu cosets of the transform", coset_begin, coset_count, all_cosets);
    if (d == 0) {                                           // constants: every evaluation equals them
        for (size_t k = 0; k < batch + n_polys; ++k) {
            rc = x_add_lde_dev<F>(k < batch ? d_evals + F::W * k : d_coeffs[k - batch], k < batch ? 1 : n_coeffs, basis, m, shift, coset_begin, coset_count, d_outs[k]);
            if (rc != IOPX_OK) return rc;
        }
        return IOPX_OK;
    }
    std::shared_ptr<AddPlanX<F>> pl;
    rc = get_plan_x<F>(basis, d, &pl);
    if (rc != IOPX_OK) return rc;
    const size_t total = batch + n_polys;
    TmpBuf drs, dptrs, work;
    rc = upload_rs2_x(*pl, eval_shift, shift, basis + F::W * (size_t)d, nhi, drs);
    if (rc != IOPX_OK) return rc;
    bool ptrs_a16;
    rc = upload_ptrs_x(d_outs, total, d_coeffs, n_polys, dptrs, &ptrs_a16);
    if (rc != IOPX_OK) return rc;
    rc = work.alloc(total * nd * EB);
    if (rc != IOPX_OK) return rc;
    const uint64_t *const *dev_outs = (const uint64_t *const *)dptrs.u64();
    rc = run_phase2_inv_batch_x(*pl, d_evals, work.u64(), drs.u64(), batch);           // H's butterflies undone: natural order -> block order
    if (rc != IOPX_OK) return rc;
    if (n_polys) {
        uint64_t *P = work.u64() + F::W * batch * nd;
        IOPX_LAUNCHX(al16(P) && ptrs_a16, "pad_copy_batch", 0, kx_pad_copy_batch, dim3(grid_x(nd, 256), (unsigned)n_polys), dim3(256), 0, P, dev_outs + total, n_coeffs, nd);
        rc = run_phase1_batch_x<F, false>(*pl, P, n_polys);
        if (rc != IOPX_OK) return rc;
    }
    return run_phase2_fwd_batch_x(*pl, work.u64(), total, dev_outs, ptrs_a16, drs.u64() + F::W * (size_t)d, nhi, coset_begin, coset_count);
}

template<class F>
static int x_add_reextend_batch_dev(const uint64_t *d_evals, size_t batch, const uint64_t *basis, size_t m, size_t d_dim, const uint64_t *eval_shift,
                                    const uint64_t *shift, size_t coset_begin, size_t coset_count, uint64_t *const *d_outs)
{
    return x_add_reextend_lde_batch_dev<F>(d_evals, batch, nullptr, 0, 0, basis, m, d_dim, eval_shift, shift, coset_begin, coset_count, d_outs);
}

// Two groups of evaluation vectors over cosets of the same span with different shifts (f_Az, f_Bz, f_Cz over H and f_w over the first coset of V inside
// L), re-extended in ONE batch: each group's butterflies are undone with its own recursed shift, every forward launch runs over all batch_a + batch_b
// vectors; no phase-1 launch in either direction.  d_outs: group a's codewords, then group b's; bit for bit the two one-group calls'.  The three
// recursed shifts travel in one table, each section starting at an even word: rs_a, rs_b, then rs_L with L's coset basis behind it.
template<class F>
static int x_add_reextend2_batch_dev(const uint64_t *d_evals_a, size_t batch_a, const uint64_t *eval_shift_a, const uint64_t *d_evals_b, size_t batch_b,
                                     const uint64_t *eval_shift_b, const uint64_t *basis, size_t m, size_t d_dim, const uint64_t *shift, size_t coset_begin,
                                     size_t coset_count, uint64_t *const *d_outs)
{
    typedef typename F::host H;
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    rc = check_basis_args_x(basis, m, shift);
    if (rc != IOPX_OK) return rc;
    if (!d_evals_a || !d_evals_b || !d_outs || !eval_shift_a || !eval_shift_b) return fail(IOPX_ERR_INVALID_ARGUMENT, "null buffer");
    if (batch_a == 0 || batch_b == 0 || batch_a > 65535 || batch_b > 65535 || batch_a + batch_b > 65535)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "batch sizes %zu + %zu outside 1..65535", batch_a, batch_b);
    if (d_dim == 0 || d_dim > m) return fail(IOPX_ERR_INVALID_ARGUMENT, "the evaluation domains must be spanned by the first basis vectors of the codeword domain");
    const size_t total = batch_a + batch_b;
    for (size_t k = 0; k < total; ++k) if (!d_outs[k]) return fail(IOPX_ERR_INVALID_ARGUMENT, "null buffer");
    const int d = (int)d_dim, nhi = (int)m - d;
    const size_t all_cosets = (size_t)1 << nhi, nd = (size_t)1 << d;
    if (coset_count == 0 || coset_begin >= all_cosets || coset_count > all_cosets - coset_begin)
        return fail(IOPX_ERR_INVALID_ARGUMENT, "coset range [%zu, +%zu) outside the %zu cosets of the transform", coset_begin, coset_count, all_cosets);
    std::shared_ptr<AddPlanX<F>> pl;
    rc = get_plan_x<F>(basis, d, &pl);
    if (rc != IOPX_OK) return rc;
    TmpBuf drs, dptrs, work;
    const size_t section = ((size_t)d * F::W + 1) & ~(size_t)1;
    {
        std::vector<uint64_t> rs(2 * section + (size_t)(1 + nhi) * d * F::W, 0);
        pl->recurse(H(eval_shift_a), rs.data());
        pl->recurse(H(eval_shift_b), rs.data() + section);
        pl->recurse(H(shift), rs.data() + 2 * section);
        for (int v = 0; v < nhi; ++v) pl->recurse(H(basis + F::W * (size_t)(d + v)), rs.data() + 2 * section + (size_t)(1 + v) * d * F::W);
        if ((rc = drs.alloc(rs.size() * 8)) != IOPX_OK) return rc;
        if ((rc = upload(drs.p, rs.data(), rs.size() * 8)) != IOPX_OK) return rc;
    }
    bool ptrs_a16;
    rc = upload_ptrs_x(d_outs, total, nullptr, 0, dptrs, &ptrs_a16);
    if (rc != IOPX_OK) return rc;
    rc = work.alloc(total * nd * EB);
    if (rc != IOPX_OK) return rc;
    rc = run_phase2_inv_batch_x(*pl, d_evals_a, work.u64(), drs.u64(), batch_a);                                       // each group's butterflies undone: natural -> block order
    if (rc != IOPX_OK) return rc;
    rc = run_phase2_inv_batch_x(*pl, d_evals_b, work.u64() + F::W * batch_a * nd, drs.u64() + section, batch_b);
    if (rc != IOPX_OK) return rc;
    return run_phase2_fwd_batch_x(*pl, work.u64(), total, (const uint64_t *const *)dptrs.u64(), ptrs_a16, drs.u64() + 2 * section, nhi, coset_begin, coset_count);
}

template<class F>
static int x_add_fft_host(const uint64_t *coeffs, size_t n_coeffs, const uint64_t *basis, size_t m,
                          const uint64_t *shift, uint64_t *out)
{
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    rc = check_basis_args_x(basis, m, shift);
    if (rc != IOPX_OK) return rc;
    const size_t n = (size_t)1 << m;
    if (n_coeffs > n) return fail(IOPX_ERR_INVALID_ARGUMENT, "additive FFT: %zu coefficients exceed the domain size %zu", n_coeffs, n);
    if (!out || (n_coeffs && !coeffs)) return fail(IOPX_ERR_INVALID_ARGUMENT, "null buffer");
    DevBuf din, dout;
    if ((rc = din.alloc(n_coeffs * EB)) != IOPX_OK) return rc;
    if ((rc = dout.alloc(n * EB)) != IOPX_OK) return rc;
    if (n_coeffs) IOPX_HIP(copy_h2d(din.p, coeffs, n_coeffs * EB, stream()));
    rc = x_add_fft_dev<F>(n_coeffs ? din.u64() : nullptr, n_coeffs, basis, m, shift, dout.u64());
    if (rc != IOPX_OK) return rc;
    IOPX_HIP(copy_d2h(out, dout.p, n * EB, stream()));
    IOPX_HIP(hipStreamSynchronize(stream()));
    return IOPX_OK;
}

template<class F>
static int x_add_ifft_host(const uint64_t *evals, const uint64_t *basis, size_t m, const uint64_t *shift,
                           uint64_t *out)
{
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    rc = check_basis_args_x(basis, m, shift);
    if (rc != IOPX_OK) return rc;
    if (!evals || !out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null buffer");
    const size_t n = (size_t)1 << m;
    DevBuf din, dout;
    if ((rc = din.alloc(n * EB)) != IOPX_OK) return rc;
    if ((rc = dout.alloc(n * EB)) != IOPX_OK) return rc;
    IOPX_HIP(copy_h2d(din.p, evals, n * EB, stream()));
    rc = x_add_ifft_dev<F>(din.u64(), basis, m, shift, dout.u64());
    if (rc != IOPX_OK) return rc;
    IOPX_HIP(copy_d2h(out, dout.p, n * EB, stream()));
    IOPX_HIP(hipStreamSynchronize(stream()));
    return IOPX_OK;
}

// evaluate_next_f_i_over_entire_domain for affine subspaces (fri_aux.tcc:5-34 -> :36-103)
template<class F>
static int x_fri_fold_add_dev(const uint64_t *d_f_i, const uint64_t *basis, size_t m, const uint64_t *shift,
                              size_t coset_size, const uint64_t *x_i, uint64_t *d_next)
{
    typedef typename F::host H;
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension %zu too large", m);
    if (!d_f_i || !d_next || !shift || !x_i || (m && !basis)) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (coset_size == 0 || (coset_size & (coset_size - 1))) return fail(IOPX_ERR_INVALID_ARGUMENT, "coset size %zu is not a power of two", coset_size);
    const int eta = (int)ceil_log2(coset_size);
    if ((size_t)eta > m) return fail(IOPX_ERR_INVALID_ARGUMENT, "coset size %zu exceeds the domain size", coset_size);
    const size_t n = (size_t)1 << m;
    if (eta == 0) return copy_d2d(d_next, d_f_i, n * EB);     // cosets of one element: the interpolant is the constant f(v)

    std::vector<H> b(m);
    for (size_t i = 0; i < m; ++i) b[i] = H(basis + F::W * i);
    H s(shift), x(x_i);
    // constants of all eta levels, uploaded once
    std::vector<uint64_t> hc;
    std::vector<size_t> off(eta);
    for (int e = 0; e < eta; ++e) {
        if (b[0].is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "FRI fold: basis vectors are linearly dependent");
        const H b0 = b[0], b0inv = b0.inverse();
        off[e] = hc.size();
        push_words<H, F::W>(hc, (x + s) * b0inv);
        for (size_t k = 1; k < b.size(); ++k) push_words<H, F::W>(hc, b[k] * b0inv);
        // derived domain: q(X) = X^2 + b0 X
        std::vector<H> nb;
        for (size_t k = 1; k < b.size(); ++k) nb.push_back(b[k].squared() + b0 * b[k]);
        s = s.squared() + b0 * s;
        x = x.squared() + b0 * x;
        b.swap(nb);
    }
    TmpBuf dc;
    if ((rc = dc.alloc(hc.size() * 8)) != IOPX_OK) return rc;
    if ((rc = upload(dc.p, hc.data(), hc.size() * 8)) != IOPX_OK) return rc;

    // launches of up to three levels each; intermediate vectors in temporaries
    TmpBuf tmp[2];
    const uint64_t *src = d_f_i;
    size_t cur = n;
    int which = 0;
    for (int e = 0; e < eta;) {
        const int step = std::min(FOLDX_MAX_ETA, eta - e);
        const size_t n_out = cur >> step;
        uint64_t *dst = d_next;
        if (e + step != eta) {
            if ((rc = tmp[which].alloc(n_out * EB)) != IOPX_OK) return rc;
            dst = tmp[which].u64();
            which ^= 1;
        }
        FoldParamsX fp;
        memset(&fp, 0, sizeof(fp));
        fp.src = src; fp.dst = dst; fp.n_out = n_out;
        for (int t = 0; t < step; ++t) { fp.consts[t] = dc.u64() + off[e + t]; fp.nbits[t] = (int)m - 1 - (e + t); }
        const int grid = grid_x(n_out, 256);
        const bool a16 = al16(src) && al16(dst) && al16(dc.p);      // every level's constants start at an even word of dc
        if (step == 1) IOPX_LAUNCHX(a16, "fri_fold", (cur + n_out) * EB, kx_fri_fold1, dim3(grid), dim3(256), 0, fp);
        else if (step == 2) IOPX_LAUNCHX(a16, "fri_fold", (cur + n_out) * EB, kx_fri_fold2, dim3(grid), dim3(256), 0, fp);
        else IOPX_LAUNCHX(a16, "fri_fold", (cur + n_out) * EB, kx_fri_fold3, dim3(grid), dim3(256), 0, fp);
        src = dst;
        cur = n_out;
        e += step;
    }
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;                                 // constants / temporaries are released in stream order
}

template<class F>
static int x_fri_fold_add_host(const uint64_t *f_i, const uint64_t *basis, size_t m, const uint64_t *shift,
                               size_t coset_size, const uint64_t *x_i, uint64_t *next)
{
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension %zu too large", m);
    if (!f_i || !next) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (coset_size == 0 || (coset_size & (coset_size - 1)) || coset_size > ((size_t)1 << m))
        return fail(IOPX_ERR_INVALID_ARGUMENT, "bad coset size %zu", coset_size);
    const size_t n = (size_t)1 << m, n_out = n / coset_size;
    DevBuf din, dout;
    if ((rc = din.alloc(n * EB)) != IOPX_OK) return rc;
    if ((rc = dout.alloc(n_out * EB)) != IOPX_OK) return rc;
    IOPX_HIP(copy_h2d(din.p, f_i, n * EB, stream()));
    rc = x_fri_fold_add_dev<F>(din.u64(), basis, m, shift, coset_size, x_i, dout.u64());
    if (rc != IOPX_OK) return rc;
    IOPX_HIP(copy_d2h(next, dout.p, n_out * EB, stream()));
    IOPX_HIP(hipStreamSynchronize(stream()));
    return IOPX_OK;
}

// FRI_protocol::compute_domains, additive branch (libiop/protocols/ldt/fri/fri_ldt.tcc:310-338): L^(i+1) has basis q(basis[eta_i..])
// and shift q(shift), q = the subspace polynomial of span(basis[0..eta_i)).  Host-only metadata.
template<class F>
static int x_fri_domains(const uint64_t *basis, size_t m, const uint64_t *shift, const size_t *localization, size_t num_reductions,
                         uint64_t *out_bases, uint64_t *out_shifts)
{
    typedef typename F::host H;
    if ((m > 0 && !basis) || !shift || (num_reductions > 0 && (!localization || !out_bases || !out_shifts))) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<H> b(m);
    for (size_t i = 0; i < m; ++i) b[i] = H(basis + F::W * i);
    H s(shift);
    size_t off = 0;
    for (size_t r = 0; r < num_reductions; ++r) {
        const size_t eta = localization[r];
        if (eta > b.size()) return fail(IOPX_ERR_INVALID_ARGUMENT, "localization parameters exceed the domain dimension");
        const SubspacePolyX<H> q(b.data(), eta);
        std::vector<H> nb;
        for (size_t k = eta; k < b.size(); ++k) nb.push_back(q.eval(b[k]));
        s = q.eval(s);
        b.swap(nb);
        for (const H &v : b) { v.store(out_bases + F::W * off); ++off; }
        s.store(out_shifts + F::W * r);
    }
    return IOPX_OK;
}

// combined_LDT_virtual_oracle::evaluated_contents over the affine subspace (ldt_reducer_aux.tcc:39-131; constructor and
// set_random_coefficients :3-37)
template<class F>
static int x_ldt_combine_dev(const void *const *d_oracles, size_t num_oracles, const size_t *degrees,
                             const uint64_t *random_coefficients, const uint64_t *basis, size_t m, const uint64_t *shift,
                             uint64_t *d_out)
{
    typedef typename F::host H;
    const size_t EB = sizeof(typename F::mem);
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!d_oracles || !random_coefficients || !d_out || (m > 0 && !basis) || !shift) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (m > 40) return fail(IOPX_ERR_INVALID_ARGUMENT, "domain dimension %zu too large", m);
    if (!degrees || num_oracles == 0) return fail(IOPX_ERR_INVALID_ARGUMENT, "Expected same number of evaluations as in registration.");
    // the bookkeeping of the constructor + set_random_coefficients: c = {1, random...}; oracle k takes c[k] and, as the i-th submaximal
    // one, c[num + i] on its copy shifted by x^(max_degree - degree_k)
    const size_t max_degree = *std::max_element(degrees, degrees + num_oracles);
    auto coef = [&](size_t t) { return t == 0 ? H::one() : H(random_coefficients + F::W * (t - 1)); };
    struct Entry { uint64_t ptr; H own, shifted; uint64_t expo; };
    std::vector<Entry> ent;
    uint64_t all = 0;
    size_t sub = 0;
    bool a16 = al16(d_out);
    for (size_t k = 0; k < num_oracles; ++k) {
        Entry e;
        e.ptr = (uint64_t)(uintptr_t)d_oracles[k];
        a16 = a16 && al16(d_oracles[k]);
        e.own = coef(k);
        e.expo = max_degree - degrees[k];
        e.shifted = e.expo ? coef(num_oracles + sub++) : H::zero();
        all |= e.expo;
        ent.push_back(e);
    }
    std::stable_sort(ent.begin(), ent.end(), [](const Entry &a, const Entry &b) { return a.expo < b.expo; });      // groups of one exponent
    int nbits = 0;
    while (nbits < 64 && (all >> nbits)) ++nbits;
    // basis[k]^(2^i), shift^(2^i) by repeated squaring (exponentiation.tcc:10-18): depends on the domain and the exponent bits only, kept per domain
    TmpBuf dtab, dmeta;
    {
        std::vector<uint64_t> key(basis, basis + F::W * m);
        key.insert(key.end(), shift, shift + F::W);
        key.push_back(m); key.push_back((uint64_t)nbits); key.push_back(F::LDT_TAG);
        rc = cached_domain_table(key, [&](std::vector<uint64_t> &htab) -> int {
            std::vector<H> cur;
            cur.push_back(H(shift));
            for (size_t k = 0; k < m; ++k) cur.push_back(H(basis + F::W * k));
            for (int i = 0; i < (nbits ? nbits : 1); ++i) {
                for (const H &v : cur) push_words<H, F::W>(htab, v);
                for (H &v : cur) v = v.squared();
            }
            return IOPX_OK;
        }, dtab);
        if (rc != IOPX_OK) return rc;
    }
    // the per-call tables travel in one block: coefficient pairs first (whole elements), then the exponents and the oracle pointers
    const size_t CW = 2 * F::W;                     // words of one coefficient pair
    std::vector<uint64_t> meta((CW + 2) * num_oracles);
    for (size_t k = 0; k < num_oracles; ++k) {
        ent[k].own.store(&meta[CW * k]);
        ent[k].shifted.store(&meta[CW * k + F::W]);
        meta[CW * num_oracles + k] = ent[k].expo;
        meta[(CW + 1) * num_oracles + k] = ent[k].ptr;
    }
    if ((rc = dmeta.alloc(meta.size() * 8)) != IOPX_OK) return rc;
    if ((rc = upload(dmeta.p, meta.data(), meta.size() * 8)) != IOPX_OK) return rc;
    LdtParamsX p;
    p.coef = dmeta.u64(); p.expo = dmeta.u64() + CW * num_oracles;
    p.oracles = (const uint64_t *const *)(dmeta.u64() + (CW + 1) * num_oracles);
    p.out = d_out; p.tab = dtab.u64();
    p.n = (size_t)1 << m; p.m = (int)m; p.num_oracles = (int)num_oracles;
    a16 = a16 && al16(dmeta.p) && al16(dtab.p);
    IOPX_LAUNCHX(a16, "ldt_combine", (num_oracles + 1) * EB * p.n, kx_ldt_combine, dim3(grid_x(p.n, 256)), dim3(256), 0, p);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int x_mul_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (count == 0) return IOPX_OK;
    if (!d_a || !d_b || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    IOPX_LAUNCHX(al16(d_a) && al16(d_b) && al16(d_out), "mul", 0, kx_mul, dim3(grid_x(count, 256)), dim3(256), 0, d_a, d_b, d_out, count);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int x_inv_dev(const uint64_t *d_a, uint64_t *d_out, size_t count)
{
    int rc = ensure_device();
    if (rc != IOPX_OK) return rc;
    if (count == 0) return IOPX_OK;
    if (!d_a || !d_out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    IOPX_LAUNCHX(al16(d_a) && al16(d_out), "inv", 0, kx_inv, dim3(grid_x(count, 256)), dim3(256), 0, d_a, d_out, count);
    IOPX_HIP(hipGetLastError());
    return IOPX_OK;
}

template<class F>
static int x_host_mul(const uint64_t *a, const uint64_t *b, uint64_t *out)
{
    typedef typename F::host H;
    if (!a || !b || !out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    (H(a) * H(b)).store(out);
    return IOPX_OK;
}

template<class F>
static int x_inverse_host(const uint64_t *x, uint64_t *out)
{
    typedef typename F::host H;
    if (!x || !out) return fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (H(x).is_zero()) return fail(IOPX_ERR_INVALID_ARGUMENT, "inverse of zero");
    H(x).inverse().store(out);
    return IOPX_OK;
}

} // namespace iopx
