// TEST INFRASTRUCTURE ONLY: the fifteen entries of include/libiop_amd_fractal.h (gfx_ops.h) in a stand-alone program over the CPU build, for
// AddressSanitizer and UBSan (make -f gfx_fractal_selfcheck.mk gfx_fractal_selfcheck_san && ./gfx_fractal_selfcheck_san; nothing is loaded into
// Python, nothing preloaded).  What no comparison of outputs sees, because the values involved are never stored: a 16-byte access at an address that
// is only 8-byte aligned (an entry that takes the 128-bit or the pair form although one of its vectors is off the boundary), a read past a
// subset-sum table or the per-coset inverse table at the edge sizes, a step outside the batch division's product tree or the Euclid's words.  Every
// entry runs with each of its vectors in turn 8 bytes past a 16-byte boundary, at m = 0, k = 0 and k = m besides the ordinary shapes.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/libiop_amd.h"

#define CK(x) do { int rc_ = (x); if (rc_ != IOPX_OK) { std::fprintf(stderr, "%s -> %d: %s\n", #x, rc_, iopx_last_error()); return 2; } } while (0)

#define ENTRIES(F) { iopx_##F##_div_dev, iopx_domain_offsets_##F##_dev, iopx_vanishing_evals_##F##_dev, iopx_rational_combine_##F##_dev, \
                     iopx_rational_sumcheck_constraint_##F##_dev }

struct Entries {
    decltype(&iopx_gf128_div_dev) div; decltype(&iopx_domain_offsets_gf128_dev) offsets; decltype(&iopx_vanishing_evals_gf128_dev) evals;
    decltype(&iopx_rational_combine_gf128_dev) combine; decltype(&iopx_rational_sumcheck_constraint_gf128_dev) constraint;
};

static int run(const Entries &e, size_t W)
{
    const size_t m = 9, n = (size_t)1 << m, NV = 10, LONG = 256 * 16 * 2 + 3;       // eight inputs, two outputs; LONG: three ragged workgroups of the division
    std::vector<uint64_t> host(W * (LONG + NV));
    for (size_t i = 0; i < host.size(); ++i) host[i] = 0x9E3779B97F4A7C15ull * (i + 1);
    for (size_t w = 0; w < W; ++w) host[W * 7 + w] = 0;                             // a zero denominator in every vector
    void *block[NV];
    for (size_t v = 0; v < NV; ++v) CK(iopx_malloc(&block[v], 8 * W * LONG + 32));
    std::vector<uint64_t> basis(W * m, 0), shift(W, 0), kshift(W, 0), other(W * 4, 0), mu(W, 0);
    for (size_t k = 0; k < m; ++k) basis[W * k] = (uint64_t)1 << k;
    shift[0] = 0x1234567 | ((uint64_t)1 << m); shift[W - 1] |= (uint64_t)1 << 63;
    for (size_t k = 0; k < 4; ++k) other[W * k] = 0x777 * (k + 1) | ((uint64_t)1 << (20 + k));
    mu[0] = 0xABCDEF;
    // which == NV: every vector on the boundary
    for (size_t which = 0; which <= NV; ++which) {
        uint64_t *p[NV];
        for (size_t v = 0; v < NV; ++v) {
            uintptr_t u = (uintptr_t)block[v];
            u += (16 - u % 16) % 16;
            p[v] = (uint64_t *)(u + (v == which ? 8 : 0));
            CK(iopx_memcpy_h2d(p[v], host.data() + W * v, 8 * W * LONG));
        }
        for (int way = 0; way <= 2; ++way) {                    // the root's inversion: the field's choice, the Fermat power, the binary Euclid
            CK(iopx_set_option("IOPX_GFX_DIV_INVERSION", way));
            for (size_t count : { (size_t)1, (size_t)2, (size_t)255, (size_t)257, LONG }) {
                CK(e.div(p[0], p[1], p[8], count));
                CK(e.div(nullptr, p[1], p[8], count));
            }
        }
        CK(iopx_clear_option("IOPX_GFX_DIV_INVERSION"));
        for (size_t dim : { (size_t)0, (size_t)1, m }) {
            CK(e.offsets(dim ? basis.data() : nullptr, dim, shift.data(), mu.data(), p[8]));
            for (size_t vdim : { (size_t)0, (size_t)1, (size_t)4 }) {
                CK(e.evals(dim ? basis.data() : nullptr, dim, shift.data(), vdim ? other.data() : nullptr, vdim, kshift.data(), mu.data(), p[8]));
                if (vdim <= dim) CK(e.evals(dim ? basis.data() : nullptr, dim, shift.data(), vdim ? basis.data() : nullptr, vdim, kshift.data(), mu.data(), p[8]));
            }
        }
        const void *N[4] = { p[0], p[1], p[2], p[3] }, *D[4] = { p[4], p[5], p[6], p[7] };
        for (size_t num = 1; num <= 4; ++num)
            for (size_t count : { (size_t)1, (size_t)2, (size_t)257 }) CK(e.combine(N, D, num, other.data(), count, p[8], p[9]));
        for (size_t k : { (size_t)0, (size_t)1, (size_t)4, (size_t)6, m }) {
            CK(e.constraint(p[0], p[1], p[2], p[3], basis.data(), m, shift.data(), k, kshift.data(), mu.data(), p[8]));
            CK(e.constraint(p[0], p[1], p[2], p[3], basis.data(), m, shift.data(), k, kshift.data(), kshift.data(), p[8]));      // claimed sum zero
        }
        CK(e.constraint(p[0], p[1], p[2], p[3], nullptr, 0, shift.data(), 0, kshift.data(), mu.data(), p[8]));                  // m = 0: one element
        CK(e.constraint(p[0], p[1], p[2], p[3], basis.data(), 1, shift.data(), 1, kshift.data(), mu.data(), p[8]));             // the pair form's only pair
        CK(iopx_synchronize());
    }
    for (size_t v = 0; v < NV; ++v) CK(iopx_free(block[v]));
    return 0;
}

int main()
{
    CK(iopx_init(0));
    const Entries e64 = ENTRIES(gf64), e128 = ENTRIES(gf128), e256 = ENTRIES(gf256);
    int rc = run(e64, 1);
    if (rc == 0) rc = run(e128, 2);
    if (rc == 0) rc = run(e256, 4);
    CK(iopx_clear_plans());
    if (rc == 0) std::printf("gfx fractal edges ok\n");
    return rc;
}
