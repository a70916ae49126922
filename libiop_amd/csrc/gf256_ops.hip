// GF(2^256) on gfx950: the protocol-layer steps of the encoded Aurora prover (iopx_*_gf256_dev: the powers of a base, linear combinations, CSR
// matrix x vector, lincheck, rowcheck, fz, the sumcheck g oracle, division by a vanishing polynomial).  The kernels, the host code and the
// bodies of the entries are gfx_ops.h, instantiated here for Elem256; the profile reports them as k256_* (k256_*_w64 where a pointer of the
// launch is not 16-byte aligned).
#include <hip/hip_runtime.h>
#include "gf256_elem.h"
#include "runtime.h"

#include "gfx_ops.h"

IOPX_GFX_OPS_ENTRIES(gf256, iopx::Elem256)
