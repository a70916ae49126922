// TEST INFRASTRUCTURE ONLY — toy kernels that tell whether the threaded mode of the emulation (emu_runtime.cpp) detects what it claims to:
// each exists with and without the barrier it needs, and tests/test_thread_orders_selfcheck_emu.py holds which thread orders must give the
// right bytes and which must not.  Neighbour indices are clamped, not wrapped, so that every dependence points one way in thread index: with a
// wrap, thread 0 would depend on thread n - 1 and both orders would see the missing barrier of either direction.
#include <hip/hip_runtime.h>
#include "../../libiop_amd/csrc/runtime.h"

// (namespace iopx: the block-scope `extern __shared__ ... iopx_smem[]` names the enclosing namespace's variable, as in the product sources)
namespace iopx {

static __device__ uint64_t toy_a(int i) { return 0x1000 + 7 * (uint64_t)i; }
static __device__ uint64_t toy_b(int i) { return 0x900000 + 13 * (uint64_t)i; }

struct ToyParams { uint64_t *out; int barrier, n; };

// write s[tid], read the slot of the thread above
static __global__ void k_toy_read_next(ToyParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t iopx_smem[];
    const int tid = threadIdx.x, n = blockDim.x;
    iopx_smem[tid] = toy_a(tid);
    if (p.barrier) __syncthreads();
    p.out[tid] = iopx_smem[tid + 1 < n ? tid + 1 : tid];
}

// write s[tid], read the slot of the thread below
static __global__ void k_toy_read_prev(ToyParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t iopx_smem[];
    const int tid = threadIdx.x;
    iopx_smem[tid] = toy_a(tid);
    if (p.barrier) __syncthreads();
    p.out[tid] = iopx_smem[tid > 0 ? tid - 1 : 0];
}

// the partner is always in another wavefront
static __global__ void k_toy_read_other_wave(ToyParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t iopx_smem[];
    const int tid = threadIdx.x;
    iopx_smem[tid] = toy_a(tid);
    if (p.barrier) __syncthreads();
    p.out[tid] = iopx_smem[tid ^ 64];
}

// read the slot of the thread above, which that thread then overwrites: the barrier under test stands between the read and the write
static __global__ void k_toy_read_then_overwrite(ToyParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t iopx_smem[];
    const int tid = threadIdx.x, n = blockDim.x;
    iopx_smem[tid] = toy_a(tid);
    __syncthreads();
    const uint64_t seen = iopx_smem[tid + 1 < n ? tid + 1 : tid];
    if (p.barrier) __syncthreads();
    iopx_smem[tid] = toy_b(tid);
    __syncthreads();
    p.out[tid] = seen + iopx_smem[tid];
}

// in place across workgroups: the first adds to the lower half of the buffer, the second copies the lower half to the upper
static __global__ void k_toy_two_groups(ToyParams p)
{
    for (int i = threadIdx.x; i < p.n; i += blockDim.x) {       // a strided loop: one thread per workgroup shows the workgroup order too
        if (blockIdx.x == 0) p.out[i] += toy_b(i);
        else p.out[p.n + i] = p.out[i];
    }
}

// odd threads pass one barrier, even threads two
static __global__ void k_toy_skipped_barrier(ToyParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t iopx_smem[];
    const int tid = threadIdx.x;
    iopx_smem[tid] = toy_a(tid);
    __syncthreads();
    if (!(tid & 1)) __syncthreads();
    p.out[tid] = iopx_smem[tid];
}

} // namespace iopx
using namespace iopx;

// out: n words (2 n for which = 4, which the caller fills with toy_a(i) in the lower half).  Returns 0, or -1 for a kernel that does not exist.
extern "C" int iopx_emu_toy(int which, int barrier, int n, uint64_t *out)
{
    if (n < 1 || n > 1024 || (which == 2 && n != 128)) return -1;
    const ToyParams p = { out, barrier, n };
    const size_t lds = (size_t)n * sizeof(uint64_t);
    switch (which) {
    case 0: hipLaunchKernelGGL(k_toy_read_next, dim3(1), dim3(n), lds, 0, p); break;
    case 1: hipLaunchKernelGGL(k_toy_read_prev, dim3(1), dim3(n), lds, 0, p); break;
    case 2: hipLaunchKernelGGL(k_toy_read_other_wave, dim3(1), dim3(n), lds, 0, p); break;
    case 3: hipLaunchKernelGGL(k_toy_read_then_overwrite, dim3(1), dim3(n), lds, 0, p); break;
    case 4: hipLaunchKernelGGL(k_toy_two_groups, dim3(2), dim3(n), 0, 0, p); break;
    case 5: hipLaunchKernelGGL(k_toy_skipped_barrier, dim3(1), dim3(n), lds, 0, p); break;
    default: return -1;
    }
    (void)hipDeviceSynchronize();
    return 0;
}

// The memory-check mode's self-check (tests/memory_contract_cases.py check_checker_checks_itself): a TmpBuf of n bytes and, as asked, a write
// of n + 8 bytes into it (what = 0), a write of 8 bytes in front of it (1) or a read of its first word, which nobody wrote (2, into *word).
// Both writes stay inside the block's own guards, so the entry refuses to run with the mode off.  The guards are checked when the TmpBuf
// goes out of scope.
extern "C" int iopx_emu_mem_check_toy(int what, size_t n, uint64_t *word)
{
    int rc = iopx::ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!iopx::mem_check_enabled() || n < 8 || what < 0 || what > 2) return -1;
    iopx::TmpBuf t;
    if ((rc = t.alloc(n)) != IOPX_OK) return rc;
    uint8_t *p = (uint8_t *)t.p;
    if (what == 0) return iopx::fill_bytes(p, 0x11, n + 8);
    if (what == 1) return iopx::fill_bytes(p - 8, 0x11, 8);
    return word ? iopx::download(word, p, 8) : -1;
}
