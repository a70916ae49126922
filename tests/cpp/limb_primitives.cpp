// TEST INFRASTRUCTURE ONLY: the limb primitives of libiop_amd/csrc/fp3_dev.h and bn254_dev.h on raw limb vectors, compiled for the CPU with the
// fake HIP header of tests/emu, so that tests/test_limb_primitives_emu.py can hold each one to its written contract with Python integers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fp3_dev.h"
#include "bn254_dev.h"

using namespace iopx;

static fp7 f7(const uint32_t *a) { fp7 r; for (int i = 0; i < 7; ++i) r.l[i] = a[i]; return r; }
static void o7(uint32_t *o, const fp7 &v) { for (int i = 0; i < 7; ++i) o[i] = v.l[i]; }
static bn9 b9(const uint32_t *a) { bn9 r; for (int i = 0; i < 9; ++i) r.l[i] = a[i]; return r; }
static void o9(uint32_t *o, const bn9 &v) { for (int i = 0; i < 9; ++i) o[i] = v.l[i]; }

extern "C" {

void t_fp7_mul(const uint32_t *a, const uint32_t *b, uint32_t *out) { o7(out, fp7_mul(f7(a), f7(b))); }

// one butterfly in place on raw limbs (no carry handling)
void t_fp7_bfly(uint32_t *x, uint32_t *y, const uint32_t *w)
{
    fp7 X = f7(x), Y = f7(y);
    fp7_bfly(X, Y, f7(w));
    o7(x, X); o7(y, Y);
}

void t_fp7_norm(const uint32_t *a, uint32_t *out) { o7(out, fp7_norm(f7(a))); }
void t_fp7_norm_pack(const uint32_t *a, uint32_t *words6) { const fp3 r = fp7_pack(fp7_norm(f7(a))); for (int i = 0; i < 6; ++i) words6[i] = r.w[i]; }
void t_fp7_unpack(const uint32_t *words6, uint32_t *out) { fp3 a; for (int i = 0; i < 6; ++i) a.w[i] = words6[i]; o7(out, fp7_unpack(a)); }
void t_fp7_canonical(const uint32_t *a, uint32_t *words6) { const fp3 r = fp7_canonical(f7(a)); for (int i = 0; i < 6; ++i) words6[i] = r.w[i]; }
void t_fp_cond_sub_p(uint32_t *words6) { uint32_t w[6]; for (int i = 0; i < 6; ++i) w[i] = words6[i]; fp_cond_sub_p(w); for (int i = 0; i < 6; ++i) words6[i] = w[i]; }

// `terms` products accumulated, then one reduction
void t_fp7w(const uint32_t *a, const uint32_t *b, int terms, uint32_t *out)
{
    fp7w w;
    fp7w_zero(w);
    for (int t = 0; t < terms; ++t) fp7w_mac(w, f7(a + 7 * t), f7(b + 7 * t));
    o7(out, fp7w_redc(w));
}

// the group size the kernels use (lincomb, LDT combination, lincheck), so that the contract test runs exactly that many products
int t_fp7w_max_terms() { return FP7W_MAX_TERMS; }

int t_bn9_dot(int n, const uint32_t *a, const uint32_t *b, uint32_t *out)
{
    if (n == 1) { const bn9 x[1] = { b9(a) }, y[1] = { b9(b) }; o9(out, bn9_dot<1>(x, y)); return 0; }
    if (n == 3) { const bn9 x[3] = { b9(a), b9(a + 9), b9(a + 18) }, y[3] = { b9(b), b9(b + 9), b9(b + 18) }; o9(out, bn9_dot<3>(x, y)); return 0; }
    if (n == 4) { const bn9 x[4] = { b9(a), b9(a + 9), b9(a + 18), b9(a + 27) }, y[4] = { b9(b), b9(b + 9), b9(b + 18), b9(b + 27) }; o9(out, bn9_dot<4>(x, y)); return 0; }
    return -1;
}

void t_bn9_sqr(const uint32_t *a, uint32_t *out) { o9(out, bn9_sqr(b9(a))); }
void t_bn9_reduce(const uint32_t *a, uint32_t *out) { o9(out, bn9_reduce(b9(a))); }
void t_bn9_unpack(const uint64_t *q, uint32_t *out) { o9(out, bn9_unpack(q)); }
void t_bnw_add(const uint32_t *a, const uint32_t *b, uint32_t *out) { o9(out, bnw_add(b9(a), b9(b))); }
void t_bnw_sub(const uint32_t *a, const uint32_t *b, uint32_t *out) { o9(out, bnw_sub(b9(a), b9(b))); }
void t_bn9_store_canonical(const uint32_t *y, uint64_t *q) { bn9_store_canonical(q, b9(y)); }
void t_bnw_store(const uint32_t *v, uint64_t *q) { bnw_store(q, 0, b9(v)); }

} // extern "C"
