// GF(2^64) on gfx950: the protocol-layer steps of the encoded Aurora prover (iopx_*_gf64_dev: the vector add, the powers of a base, linear
// combinations, CSR matrix x vector, lincheck, rowcheck, fz, the sumcheck g oracle, division by a vanishing polynomial).  The kernels, the host
// code and the bodies of the entries are gfx_ops.h, instantiated here for Elem64.  An element is 8 bytes and a product ~0.13k VALU ops
// (gf64_dev.h): every kernel is bound by its HBM passes, so a lane of the 16-byte form takes two consecutive elements with one access.  The
// profile reports the kernels as k64_* (k64_*_w64 where a vector of the launch is not 16-byte aligned: one element per lane).
#include <hip/hip_runtime.h>
#include "gf64_elem.h"
#include "runtime.h"

#include "gfx_ops.h"

IOPX_GFX_OPS_ENTRIES(gf64, iopx::Elem64)
