// TEST INFRASTRUCTURE ONLY — a stand-in for the HIP runtime that runs kernels on the CPU.
//
// There is no GPU in the development container, so the CPU test-suite compiles the PRODUCT kernel
// sources (libiop_amd/csrc/*.hip, unmodified, no #ifdefs in them) with g++ against this header and runs
// every workgroup sequentially with blockDim = 1.  All kernels are written as block-size-agnostic
// strided loops separated by __syncthreads(), so one thread per workgroup executes the same index
// arithmetic, tile schedules and field arithmetic as the GPU does.  This validates kernel LOGIC before
// GPU time is spent; it is not shipped, not loaded by libiop_amd, and not a fallback (the product
// library links the real HIP runtime and fails without a device).
//
// That single thread cannot see a missing barrier or two wavefronts that own the same LDS row.  iopx_emu_set_threads (emu_runtime.cpp)
// switches to the threaded mode: every workgroup runs with the blockDim of its launch, one fiber per thread, each fiber alone up to its next
// __syncthreads(), in ascending, descending or a seeded order of thread index.  __shared__ is thread_local for it: all fibers of a workgroup
// run on the OS thread that launches, so a block-scope __shared__ array is storage they share (and it stays off the small fiber stacks).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <tuple>
#include <type_traits>
#include <utility>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __shared__ thread_local
#define __launch_bounds__(...)

struct dim3 {
    unsigned x, y, z;
    constexpr dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}     // constexpr: the thread_local ones below are constant-initialised
};
extern thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
struct uint4 { unsigned x, y, z, w; };
static inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { uint4 v = { x, y, z, w }; return v; }

// threaded mode: the calling fiber yields until every live fiber of its workgroup has arrived; one thread per workgroup: nothing
void __syncthreads();
// one thread at a time: a ballot sees the calling lane only
static inline unsigned long long __ballot(int pred) { return pred ? ~0ull : 0ull; }      // (the emulated thread stands for every lane of its wavefront)
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline void __threadfence_block() {}
static inline unsigned long long atomicMin(unsigned long long *p, unsigned long long v)
{
    const unsigned long long old = *p;
    if (v < old) *p = v;
    return old;
}
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v)
{
    const unsigned long long old = *p;
    *p = old + v;
    return old;
}
static inline void __threadfence() {}
static inline uint32_t __brev(uint32_t x)
{
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
}

// gfx950 builtins used by the kernels, bit-exact software models
static inline uint32_t __builtin_amdgcn_bitop3_b32(uint32_t a, uint32_t b, uint32_t c, uint32_t tt)
{
    if (tt == 0x78) return a ^ (b & c);      // fast path for the form the field multiply uses
    if (tt == 0x96) return a ^ b ^ c;
    if (tt == 0xE4) return (a & c) | (b & ~c);
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) {
        const uint32_t idx = (((a >> i) & 1) << 2) | (((b >> i) & 1) << 1) | ((c >> i) & 1);
        r |= ((tt >> idx) & 1u) << i;
    }
    return r;
}
static inline int __builtin_amdgcn_sbfe(int v, unsigned off, unsigned width)
{
    const uint32_t x = ((uint32_t)v >> off) & ((width >= 32) ? 0xFFFFFFFFu : ((1u << width) - 1));
    const uint32_t sign = 1u << (width - 1);
    return (int)((x ^ sign) - sign);
}

static inline uint32_t __builtin_amdgcn_readfirstlane(uint32_t x) { return x; }
// v_alignbit_b32: the low 32 bits of ((hi:lo) >> (s & 31))
static inline uint32_t __builtin_amdgcn_alignbit(uint32_t hi, uint32_t lo, uint32_t s)
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31));
}

static inline unsigned long long __brevll(unsigned long long x)
{
    unsigned long long r = 0;
    for (int i = 0; i < 64; ++i) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
}

typedef int hipError_t;
typedef void *hipStream_t;
enum { hipSuccess = 0, hipErrorNotReady = 600, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToHost, hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice, hipMemcpyDefault };
enum { hipStreamNonBlocking = 1 };
enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };

static inline const char *hipGetErrorString(hipError_t e) { return e == hipErrorNotReady ? "emu: not ready" : "emu"; }
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
static inline hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
static inline hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }

// Streams, events and memory live in emu_runtime.cpp.  On the default ("eager") schedule every call below acts at once, as a single
// implicit stream would; on a deferred schedule (iopx_emu_set_schedule) each stream is a queue of operations that executes only where the
// host synchronises, so that a missing ordering edge between two streams changes the bytes a test sees.
hipError_t hipSetDevice(int);
hipError_t hipDeviceSynchronize();
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags);
hipError_t hipStreamDestroy(hipStream_t s);
hipError_t hipStreamSynchronize(hipStream_t s);
hipError_t hipMalloc(void **p, size_t n);
template<typename T> static inline hipError_t hipMalloc(T **p, size_t n) { return hipMalloc((void **)p, n); }
hipError_t hipFree(void *p);
hipError_t hipMallocAsync(void **p, size_t n, hipStream_t s);
hipError_t hipFreeAsync(void *p, hipStream_t s);
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind kind, hipStream_t stream);
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t stream);

typedef void *hipEvent_t;
enum { hipEventDisableTiming = 2 };
hipError_t hipHostMalloc(void **p, size_t n, unsigned flags);
hipError_t hipHostFree(void *p);
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags);
hipError_t hipEventQuery(hipEvent_t e);
hipError_t hipEventCreate(hipEvent_t *e);
hipError_t hipEventDestroy(hipEvent_t e);
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s);
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags);
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b);

// LDS: one static buffer, the size of a CU's LDS
namespace iopx { extern thread_local uint64_t iopx_smem[]; }
// runs every workgroup of the grid now, on the calling thread (with one thread each, or in the threaded mode one fiber per thread of `block`)
void emu_launch(dim3 grid, dim3 block, size_t lds_bytes, const std::function<void()> &body);
// eager schedule: emu_launch at once; deferred: the closure joins the stream's queue and emu_launch runs it when the stream executes
void emu_enqueue_launch(hipStream_t stream, dim3 grid, dim3 block, size_t lds_bytes, std::function<void()> body);

// A launch copies its arguments when it is enqueued, converted to the kernel's parameter types as the real launch does: the caller's
// variables may change or die before the kernel runs.
template<typename... P, typename... A>
static inline std::function<void()> emu_bind(void (*kernel)(P...), A &&...args)
{
    return [kernel, held = std::tuple<typename std::decay<P>::type...>(std::forward<A>(args)...)]() { std::apply(kernel, held); };
}

#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
    emu_enqueue_launch((hipStream_t)(stream), (grid), (block), (lds), emu_bind(kernel, ##__VA_ARGS__))
