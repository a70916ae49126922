// TEST INFRASTRUCTURE ONLY: the pair-form entries of libiop_amd/csrc/gfx_ops.h over gf64 (gf64_ops.hip) in a stand-alone program over the CPU build, for
// AddressSanitizer and UBSan (make gf64_edges_selfcheck_san && ./gf64_edges_selfcheck_san; nothing is loaded into Python, nothing preloaded).
// Two things no comparison of outputs sees, because the values involved are never stored: a 16-byte access at an address that is only 8-byte
// aligned (an entry that takes the two-element form although one of its vectors is off the boundary), and the read of a subset-sum table's
// entry for bit 0 on a domain of one element, where the table has no such entry.  Every entry runs with each of its vectors in turn 8 bytes
// past a 16-byte boundary, and the domain-shaped ones at m = 0 with everything aligned.  The transform, fold and LDT entries of gf64.hip,
// which share their text with the wider fields' 16-byte elements, then run with every device pointer off the boundary.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/libiop_amd.h"

#define CK(x) do { int rc_ = (x); if (rc_ != IOPX_OK) { std::fprintf(stderr, "%s -> %d: %s\n", #x, rc_, iopx_last_error()); return 2; } } while (0)

int main()
{
    CK(iopx_init(0));
    const size_t m = 9, n = (size_t)1 << m, NV = 6;
    std::vector<uint64_t> host(n + NV);
    for (size_t i = 0; i < host.size(); ++i) host[i] = 0x9E3779B97F4A7C15ull * (i + 1);
    void *block[NV];
    for (size_t v = 0; v < NV; ++v) CK(iopx_malloc(&block[v], 8 * n + 32));
    uint64_t basis[m];
    for (size_t k = 0; k < m; ++k) basis[k] = (uint64_t)1 << k;
    const uint64_t shift = ((uint64_t)1 << 63) | 0x1234567 | ((uint64_t)1 << m), cshift = 0x55, ishift = ((uint64_t)1 << 63) | 9, zero = 0,
                   mu = ((uint64_t)1 << 63) | 77, coef[2] = { 3, ((uint64_t)1 << 63) | 5 };
    // which == NV: every vector on the boundary
    for (size_t which = 0; which <= NV; ++which) {
        uint64_t *p[NV];
        for (size_t v = 0; v < NV; ++v) {
            uintptr_t u = (uintptr_t)block[v];
            u += (16 - u % 16) % 16;
            p[v] = (uint64_t *)(u + (v == which ? 8 : 0));
            CK(iopx_memcpy_h2d(p[v], host.data() + v, 8 * n));
        }
        const void *two[2] = { p[0], p[1] }, *one[1] = { p[3] };
        CK(iopx_gf64_add_dev(p[0], p[1], p[5], n - 1));
        CK(iopx_lincomb_gf64_dev(two, 2, coef, n - 1, p[5]));
        CK(iopx_lincomb_affine_gf64_dev(two, 2, coef, &mu, n - 1, p[5]));
        CK(iopx_lincheck_gf64_dev(p[0], one, 1, coef, p[1], p[2], n - 1, p[5]));
        CK(iopx_rowcheck_gf64_dev(p[0], p[1], p[2], basis, m, &shift, 4, &cshift, p[5]));
        CK(iopx_fz_gf64_dev(p[0], p[1], basis, m, &shift, basis, 4, &ishift, p[5]));
        CK(iopx_sumcheck_g_gf64_dev(p[0], p[1], basis, m, &shift, basis, 6, &zero, &zero, p[5]));
        CK(iopx_sumcheck_g_gf64_dev(p[0], p[1], basis, m, &shift, basis, 6, &zero, &mu, p[5]));
        if (which == NV) {      // one element: the second of the pair is absent, and so is the table's entry for bit 0
            CK(iopx_rowcheck_gf64_dev(p[0], p[1], p[2], nullptr, 0, &shift, 0, &cshift, p[5]));
            CK(iopx_fz_gf64_dev(p[0], p[1], nullptr, 0, &shift, nullptr, 0, &ishift, p[5]));
            CK(iopx_sumcheck_g_gf64_dev(p[0], p[1], nullptr, 0, &shift, nullptr, 0, &ishift, &zero, p[5]));
            CK(iopx_sumcheck_g_gf64_dev(p[0], p[1], nullptr, 0, &shift, nullptr, 0, &ishift, &mu, p[5]));
        }
        CK(iopx_synchronize());
    }
    // The transform, fold and LDT entries of gf64.hip (gfx_additive.h over a one-word element) on 2^5 elements in tiles of 2^4 (chunked
    // phase 1, one upper pass, the last pass), every device pointer 8 bytes past a 16-byte boundary: a 16-byte access would be misaligned.
    {
        const char *const opts[4] = { "IOPX_GF64_TILE_BITS", "IOPX_GF64_P1_COLS", "IOPX_GF64_P2_COLS", "IOPX_GF64_P2_TOP" };
        for (int i = 0; i < 4; ++i) CK(iopx_set_option(opts[i], i == 0 ? 4 : 1));
        CK(iopx_clear_plans());
        const size_t m5 = 5, n5 = (size_t)1 << m5;
        uint64_t *p[NV];
        for (size_t v = 0; v < NV; ++v) {
            uintptr_t u = (uintptr_t)block[v];
            u += (16 - u % 16) % 16;
            p[v] = (uint64_t *)(u + 8);
            CK(iopx_memcpy_h2d(p[v], host.data() + v, 8 * n5));
        }
        const uint64_t x = ((uint64_t)1 << 62) | 0xABCDEF;
        CK(iopx_add_fft_gf64_dev(p[0], n5, basis, m5, &shift, p[4]));
        CK(iopx_add_ifft_gf64_dev(p[4], basis, m5, &shift, p[5]));
        std::vector<uint64_t> back(n5);
        CK(iopx_memcpy_d2h(back.data(), p[5], 8 * n5));
        for (size_t i = 0; i < n5; ++i) if (back[i] != host[i]) { std::fprintf(stderr, "IFFT(FFT) differs at %zu\n", i); return 2; }
        CK(iopx_add_ifft_gf64_dev(p[4], basis, m5, &shift, p[4]));                  // in place
        CK(iopx_add_lde_gf64_dev(p[0], n5, basis, 7, &shift, 1, 2, p[5]));          // cosets [1, 3) of four: the staged group
        const size_t cosets[3] = { 2, 4, 16 };                                      // one launch, one launch, two launches
        for (size_t c = 0; c < 3; ++c) CK(iopx_fri_fold_add_gf64_dev(p[0], basis, m5, &shift, cosets[c], &x, p[5]));
        const void *three[3] = { p[0], p[1], p[2] };
        const size_t degrees[3] = { n5, n5 - 3, n5 - 3 };
        const uint64_t rc[6] = { 3, ((uint64_t)1 << 63) | 5, 7, 0x1B, ((uint64_t)1 << 40) | 1, 11 };
        CK(iopx_ldt_combine_gf64_dev(three, 3, degrees, rc, basis, m5, &shift, p[5]));
        CK(iopx_synchronize());
        for (int i = 0; i < 4; ++i) CK(iopx_clear_option(opts[i]));
        CK(iopx_clear_plans());
    }
    for (size_t v = 0; v < NV; ++v) CK(iopx_free(block[v]));
    std::puts("gf64 edges: every entry ran at every placement and at m = 0");
    return 0;
}
