// GF(2^128) on gfx950: the protocol-layer steps of the encoded Aurora prover (iopx_*_gf128_dev: the powers of a base, linear combinations, CSR
// matrix x vector, lincheck, rowcheck, fz, the sumcheck g oracle, division by a vanishing polynomial).  The kernels, the host code and the
// bodies of the entries are gfx_ops.h, instantiated here for Elem128; the profile reports them as k128_* (k128_*_w64 where a pointer of the
// launch is not 16-byte aligned).
#include <hip/hip_runtime.h>
#include "gf128_elem.h"
#include "runtime.h"

#include "gfx_ops.h"

IOPX_GFX_OPS_ENTRIES(gf128, iopx::Elem128)
