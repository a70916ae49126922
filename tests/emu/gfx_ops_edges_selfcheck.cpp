// TEST INFRASTRUCTURE ONLY: the protocol-layer entries of libiop_amd/csrc/gfx_ops.h over the wider fields (gf128_ops.hip, gf256_ops.hip) in a stand-alone program over
// the CPU build, for AddressSanitizer and UBSan (make -f gfx_ops_edges_selfcheck.mk gfx_ops_edges_selfcheck_san && ./gfx_ops_edges_selfcheck_san; nothing is loaded into Python,
// nothing preloaded).  Two things no comparison of outputs sees, because the values involved are never stored: a 16-byte access at an address that
// is only 8-byte aligned (an entry that takes the 128-bit form although one of its vectors is off the boundary), and a read past a subset-sum
// table on a domain of one element.  Every entry runs with each of its vectors in turn 8 bytes past a 16-byte boundary, and the domain-shaped
// ones at m = 0.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/libiop_amd.h"

#define CK(x) do { int rc_ = (x); if (rc_ != IOPX_OK) { std::fprintf(stderr, "%s -> %d: %s\n", #x, rc_, iopx_last_error()); return 2; } } while (0)

#define ENTRIES(F) { iopx_##F##_add_dev, iopx_##F##_pow_table_dev, iopx_lincomb_##F##_dev, iopx_lincomb_affine_##F##_dev, iopx_spmv_##F##_dev, iopx_lincheck_##F##_dev, \
                     iopx_rowcheck_##F##_dev, iopx_fz_##F##_dev, iopx_sumcheck_g_##F##_dev, iopx_poly_div_vanishing_##F##_dev }

struct Entries {
    decltype(&iopx_gf128_add_dev) add; decltype(&iopx_gf128_pow_table_dev) pow_table; decltype(&iopx_lincomb_gf128_dev) lincomb;
    decltype(&iopx_lincomb_affine_gf128_dev) lincomb_affine; decltype(&iopx_spmv_gf128_dev) spmv; decltype(&iopx_lincheck_gf128_dev) lincheck;
    decltype(&iopx_rowcheck_gf128_dev) rowcheck; decltype(&iopx_fz_gf128_dev) fz; decltype(&iopx_sumcheck_g_gf128_dev) sumcheck_g;
    decltype(&iopx_poly_div_vanishing_gf128_dev) poly_div_vanishing;
};

static int run(const Entries &e, size_t W)
{
    const size_t m = 9, n = (size_t)1 << m, NV = 6;
    std::vector<uint64_t> host(W * (n + NV));
    for (size_t i = 0; i < host.size(); ++i) host[i] = 0x9E3779B97F4A7C15ull * (i + 1);
    void *block[NV], *d_rows, *d_cols;
    for (size_t v = 0; v < NV; ++v) CK(iopx_malloc(&block[v], 8 * W * n + 32));
    std::vector<uint64_t> rows(n);                       // n - 1 rows of one entry each
    std::vector<uint32_t> cols(n - 1);
    for (size_t r = 0; r < n; ++r) rows[r] = r;
    for (size_t r = 0; r + 1 < n; ++r) cols[r] = (uint32_t)((7 * r) % (n - 1));
    CK(iopx_malloc(&d_rows, 8 * n));
    CK(iopx_malloc(&d_cols, 4 * n));
    CK(iopx_memcpy_h2d(d_rows, rows.data(), 8 * n));
    CK(iopx_memcpy_h2d(d_cols, cols.data(), 4 * (n - 1)));
    std::vector<uint64_t> basis(W * m, 0), shift(W, 0), cshift(W, 0), ishift(W, 0), zero(W, 0), mu(W, 0), coef(2 * W, 0);
    for (size_t k = 0; k < m; ++k) basis[W * k] = (uint64_t)1 << k;
    shift[0] = 0x1234567 | ((uint64_t)1 << m); shift[W - 1] |= (uint64_t)1 << 63;
    cshift[0] = 0x55; ishift[0] = 9; ishift[W - 1] |= (uint64_t)1 << 63; mu[0] = 77; mu[W - 1] |= (uint64_t)1 << 63;
    coef[0] = 3; coef[W] = 5; coef[2 * W - 1] = (uint64_t)1 << 63;
    // which == NV: every vector on the boundary
    for (size_t which = 0; which <= NV; ++which) {
        uint64_t *p[NV];
        for (size_t v = 0; v < NV; ++v) {
            uintptr_t u = (uintptr_t)block[v];
            u += (16 - u % 16) % 16;
            p[v] = (uint64_t *)(u + (v == which ? 8 : 0));
            CK(iopx_memcpy_h2d(p[v], host.data() + W * v, 8 * W * (n - 1)));
        }
        const void *two[2] = { p[0], p[1] }, *one[1] = { p[3] };
        CK(e.add(p[0], p[1], p[5], n - 1));
        CK(e.pow_table(p[5], n - 1, mu.data(), coef.data()));
        CK(e.lincomb(two, 2, coef.data(), n - 1, p[5]));
        CK(e.lincomb_affine(two, 2, coef.data(), mu.data(), n - 1, p[5]));
        CK(e.spmv((const uint64_t *)d_rows, (const uint32_t *)d_cols, p[0], n - 1, p[1], mu.data(), 1, p[5]));
        CK(e.lincheck(p[0], one, 1, coef.data(), p[1], p[2], n - 1, p[5]));
        CK(e.rowcheck(p[0], p[1], p[2], basis.data(), m, shift.data(), 4, cshift.data(), p[5]));
        CK(e.fz(p[0], p[1], basis.data(), m, shift.data(), basis.data(), 4, ishift.data(), p[5]));
        CK(e.sumcheck_g(p[0], p[1], basis.data(), m, shift.data(), basis.data(), 6, zero.data(), zero.data(), p[5]));
        CK(e.sumcheck_g(p[0], p[1], basis.data(), m, shift.data(), basis.data(), 6, zero.data(), mu.data(), p[5]));
        CK(e.poly_div_vanishing(p[0], n - 1, basis.data(), 5, shift.data(), p[5]));         // several passes through a temporary
        CK(e.poly_div_vanishing(p[0], 40, basis.data(), 5, shift.data(), p[5]));            // one pass
        if (which == NV) {      // one element: the tables have their entry 0 alone
            CK(e.rowcheck(p[0], p[1], p[2], nullptr, 0, shift.data(), 0, cshift.data(), p[5]));
            CK(e.fz(p[0], p[1], nullptr, 0, shift.data(), nullptr, 0, ishift.data(), p[5]));
            CK(e.sumcheck_g(p[0], p[1], nullptr, 0, shift.data(), nullptr, 0, ishift.data(), zero.data(), p[5]));
            CK(e.sumcheck_g(p[0], p[1], nullptr, 0, shift.data(), nullptr, 0, ishift.data(), mu.data(), p[5]));
            CK(e.poly_div_vanishing(p[0], 3, nullptr, 0, shift.data(), p[5]));
            CK(e.pow_table(p[5], 1, mu.data(), coef.data()));
        }
        CK(iopx_synchronize());
    }
    for (size_t v = 0; v < NV; ++v) CK(iopx_free(block[v]));
    CK(iopx_free(d_rows));
    CK(iopx_free(d_cols));
    return 0;
}

int main()
{
    CK(iopx_init(0));
    const Entries e128 = ENTRIES(gf128), e256 = ENTRIES(gf256);
    int rc = run(e128, 2);
    if (rc == 0) rc = run(e256, 4);
    CK(iopx_clear_plans());
    if (rc == 0) std::printf("gfx ops edges ok\n");
    return rc;
}
