// TEST INFRASTRUCTURE ONLY: the nine entries of include/libiop_amd_head.h (gfx_ops.h, gfx_additive.h) in a stand-alone program over the
// CPU build, for AddressSanitizer and UBSan (make -f gfx_head_selfcheck.mk gfx_head_selfcheck_san && ./gfx_head_selfcheck_san; nothing is loaded
// into Python, nothing preloaded).  What no comparison of outputs sees, because the values involved are never stored: a 16-byte access at an address
// that is only 8-byte aligned (an entry that takes the 128-bit or the pair form although one of its vectors is off the boundary), and a read past
// the per-coset inverse table or the recursed-shift table at the edge sizes.  Every entry runs with each of its vectors in turn 8 bytes past a
// 16-byte boundary, at m = 0, sub_dim = 0 and sub_dim = m besides the ordinary shapes.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/libiop_amd.h"

#define CK(x) do { int rc_ = (x); if (rc_ != IOPX_OK) { std::fprintf(stderr, "%s -> %d: %s\n", #x, rc_, iopx_last_error()); return 2; } } while (0)

#define ENTRIES(F) { iopx_div_by_vanishing_##F##_dev, iopx_##F##_vanishing_host, iopx_add_reextend2_##F##_batch_dev }

struct Entries {
    decltype(&iopx_div_by_vanishing_gf128_dev) div; decltype(&iopx_gf128_vanishing_host) host; decltype(&iopx_add_reextend2_gf128_batch_dev) reextend2;
};

static int run(const Entries &e, size_t W)
{
    const size_t m = 9, n = (size_t)1 << m, NV = 7;          // two inputs, up to five outputs
    std::vector<uint64_t> host(W * (n + NV));
    for (size_t i = 0; i < host.size(); ++i) host[i] = 0x9E3779B97F4A7C15ull * (i + 1);
    void *block[NV];
    for (size_t v = 0; v < NV; ++v) CK(iopx_malloc(&block[v], 8 * W * n + 32));
    std::vector<uint64_t> basis(W * m, 0), shift(W, 0), sshift(W, 0), other(W, 0), value(W, 0), lin(W, 0);
    for (size_t k = 0; k < m; ++k) basis[W * k] = (uint64_t)1 << k;
    shift[0] = 0x1234567 | ((uint64_t)1 << m); shift[W - 1] |= (uint64_t)1 << 63;
    sshift[0] = 0x55; other[0] = 0x777 | ((uint64_t)1 << 20);
    // which == NV: every vector on the boundary
    for (size_t which = 0; which <= NV; ++which) {
        uint64_t *p[NV];
        for (size_t v = 0; v < NV; ++v) {
            uintptr_t u = (uintptr_t)block[v];
            u += (16 - u % 16) % 16;
            p[v] = (uint64_t *)(u + (v == which ? 8 : 0));
            CK(iopx_memcpy_h2d(p[v], host.data() + W * v, 8 * W * n));
        }
        CK(e.div(p[0], basis.data(), m, shift.data(), 4, sshift.data(), p[2]));
        CK(e.div(p[0], basis.data(), m, shift.data(), 0, sshift.data(), p[2]));            // sub_dim = 0: one inverse per element
        CK(e.div(p[0], basis.data(), m, shift.data(), m, sshift.data(), p[2]));            // sub_dim = m: one coset, one inverse
        CK(e.div(p[1], basis.data(), m, shift.data(), 4, sshift.data(), p[1]));            // in place
        CK(e.div(p[0], nullptr, 0, shift.data(), 0, sshift.data(), p[2]));                 // m = 0: one element
        CK(e.div(p[0], basis.data(), 1, shift.data(), 1, sshift.data(), p[2]));            // two elements: the pair form's only pair
        CK(e.div(p[0], basis.data(), 1, shift.data(), 0, sshift.data(), p[2]));
        // 2 + 3 vectors of 2^5 onto cosets [1, 4) of 2^7 points, 3 + 1 of 2^9 onto the single coset (m = d), 1 + 1 of 2 elements onto both cosets of 4
        uint64_t *outs5[5] = { p[2], p[3], p[4], p[5], p[6] };
        CK(e.reextend2(p[0], 2, sshift.data(), p[1], 3, shift.data(), basis.data(), 7, 5, shift.data(), 1, 3, outs5));
        CK(e.reextend2(p[0], 2, sshift.data(), p[1], 3, other.data(), basis.data(), 7, 5, shift.data(), 0, 4, outs5));
        uint64_t *outs2[2] = { p[2], p[3] };
        CK(e.reextend2(p[0], 1, sshift.data(), p[1], 1, shift.data(), basis.data(), m, m, shift.data(), 0, 1, outs2));
        CK(e.reextend2(p[0], 1, sshift.data(), p[1], 1, shift.data(), basis.data(), 2, 1, shift.data(), 0, 2, outs2));
        CK(e.reextend2(p[0], 1, sshift.data(), p[1], 1, shift.data(), basis.data(), 1, 1, shift.data(), 0, 1, outs2));
        CK(iopx_synchronize());
    }
    // the host entry: dim = 0, dim = m, either output alone
    CK(e.host(nullptr, 0, shift.data(), other.data(), value.data(), lin.data()));
    CK(e.host(basis.data(), m, shift.data(), other.data(), value.data(), nullptr));
    CK(e.host(basis.data(), m, shift.data(), other.data(), nullptr, lin.data()));
    CK(e.host(basis.data(), 4, sshift.data(), shift.data(), nullptr, nullptr));
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
    if (rc == 0) std::printf("gfx head edges ok\n");
    return rc;
}
