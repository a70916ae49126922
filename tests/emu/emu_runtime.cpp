// TEST INFRASTRUCTURE ONLY — see fakehip/hip/hip_runtime.h
//
// Besides running kernels one workgroup at a time (with one thread each or, in the threaded mode below, one fiber per thread), this file models HIP's streams and events so that a missing ordering edge between two
// streams shows as a deterministic difference in bytes ("Emulated streams").
//   eager (default)   every call acts at once: one implicit stream, the behaviour the suite has always had
//   all late          every stream is a queue of operations (launches, asynchronous copies and fills, event records, event waits) that runs
//                     only where the host synchronises: hipStreamSynchronize (that stream, and what its waits need, up to the awaited records
//                     and no further), hipDeviceSynchronize / hipFree / hipHostFree / hipSetDevice / unload (everything)
//   one stream late   the stream with the given creation index is such a queue; the others run each operation when it is enqueued (pulling
//                     the late one up to a record they wait for)
// Together: for any two streams, both extreme legal interleavings.  The legacy stream 0 (and any handle this file did not create) is a queue
// of its own; it does not synchronise with the others, which is right for hipStreamNonBlocking streams, the only kind the product creates.
#include <hip/hip_runtime.h>
#include <atomic>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include <sys/mman.h>
#include <ucontext.h>
#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/common_interface_defs.h>
#endif

thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
// thread_local like every __shared__ declaration (fakehip/hip/hip_runtime.h): the kernels' block-scope `extern __shared__ ... iopx_smem[]` names this
namespace iopx { alignas(16) thread_local uint64_t iopx_smem[160 * 1024 / 8]; }

thread_local int iopx_emu_lane = 0;

// ---- threaded mode: one fiber per thread of a workgroup --------------------------------------------------------------------------------
// order & 3: 0 one thread per workgroup (blockDim = 1, the default), 1 ascending thread index, 2 descending, 3 a permutation drawn from the seed
// and the workgroup's index; order & 4: workgroups in descending order.  A fiber runs alone until its next __syncthreads() or its return, and the
// next phase starts when every live fiber has arrived: a value that one thread writes and another reads inside one barrier interval is read
// stale under ascending or under descending order, whichever runs the reader first.
namespace {

enum { THREADS_ONE = 0, THREADS_ASC = 1, THREADS_DESC = 2, THREADS_SEEDED = 3, THREADS_GROUPS_DESC = 4 };
std::atomic<int> g_thread_order{ 0 };
std::atomic<uint64_t> g_thread_seed{ 0 };
std::atomic<long> g_barrier_mismatches{ 0 };

// Fiber stacks.  The deepest a fiber got in the whole of tests/test_thread_orders_emu.py (every kernel with a barrier, the Poseidon and prime-field
// ones among them), measured as the high-water mark of stacks filled with a pattern: 3944 bytes at -O2 and 32640 bytes with the sources built at
// -O0, as the sanitizer libraries are.  256 KiB leaves eight times the larger figure for the sanitizers' red zones; only touched pages are ever
// resident.  Below each stack lies one PROT_NONE guard page, so an overflow faults at once instead of reaching a neighbour.  Stacks are mapped
// once per OS thread, on first use, and reused by every later launch.
const size_t STACK_BYTES = 256 * 1024, GUARD_BYTES = 4096;

// The switch between a fiber and the scheduler.  On x86-64 it is twelve instructions of our own (the callee-saved registers, the two floating-point
// control words and the stack pointer): swapcontext makes a system call for the signal mask at every switch, which tripled the time of a transform
// under the threaded mode.  Anywhere else, and in the AddressSanitizer builds (which know swapcontext and are told of every switch below), ucontext.
#if defined(__x86_64__) && !defined(__SANITIZE_ADDRESS__)
#define EMU_OWN_SWITCH 1
typedef void *Context;              // the saved stack pointer
extern "C" void emu_switch(Context *save, Context load);
asm(R"(
    .pushsection .text
    .type emu_switch, @function
emu_switch:
    pushq %rbp
    pushq %rbx
    pushq %r12
    pushq %r13
    pushq %r14
    pushq %r15
    subq $8, %rsp
    stmxcsr (%rsp)
    fnstcw 4(%rsp)
    movq %rsp, (%rdi)
    movq %rsi, %rsp
    ldmxcsr (%rsp)
    fldcw 4(%rsp)
    addq $8, %rsp
    popq %r15
    popq %r14
    popq %r13
    popq %r12
    popq %rbx
    popq %rbp
    ret
    .size emu_switch, . - emu_switch
    .popsection
)");
static inline void switch_context(Context *from, Context *to) { emu_switch(from, *to); }
#else
typedef ucontext_t Context;
static inline void switch_context(Context *from, Context *to) { swapcontext(from, to); }
#endif

struct Fiber {
    Context ctx;
    char *stack = nullptr;          // lowest usable byte (the guard page lies below)
    bool done = true;
    void *asan_fake = nullptr;
};

struct Group {
    std::vector<Fiber *> fibers;    // grows to the largest block seen on this OS thread
    Context scheduler;
    const std::function<void()> *body = nullptr;
    Fiber *current = nullptr;       // the fiber that runs now; null: the scheduler (or no threaded launch at all)
    const void *sched_stack = nullptr;
    size_t sched_size = 0;
    ~Group()
    {
        for (Fiber *f : fibers) { munmap(f->stack - GUARD_BYTES, STACK_BYTES + GUARD_BYTES); delete f; }
    }
};
thread_local Group t_group;

#if defined(__SANITIZE_ADDRESS__)
#define EMU_ASAN_START(save, bottom, size) __sanitizer_start_switch_fiber(save, bottom, size)
#define EMU_ASAN_FINISH(save, bottom, size) __sanitizer_finish_switch_fiber(save, bottom, size)
#else
#define EMU_ASAN_START(save, bottom, size) ((void)0)
#define EMU_ASAN_FINISH(save, bottom, size) ((void)0)
#endif

void fiber_main()
{
    Group &g = t_group;
    EMU_ASAN_FINISH(nullptr, &g.sched_stack, &g.sched_size);
    (*g.body)();
    Fiber *f = g.current;
    f->done = true;
    EMU_ASAN_START(nullptr, g.sched_stack, g.sched_size);       // null: this fiber's frames are dead, its fake stack goes
    switch_context(&f->ctx, &g.scheduler);
    abort();                                                    // a finished fiber is never resumed: its context is made anew
}

void resume(Group &g, Fiber *f)
{
    g.current = f;
    void *fake = nullptr;
    EMU_ASAN_START(&fake, f->stack, STACK_BYTES);
    switch_context(&g.scheduler, &f->ctx);
    EMU_ASAN_FINISH(fake, nullptr, nullptr);
    (void)fake;
    g.current = nullptr;
}

// the first switch to f enters fiber_main on f's stack
void start_at_fiber_main(Fiber *f)
{
#ifdef EMU_OWN_SWITCH
    // what emu_switch pops, from the saved stack pointer up: the control words of the scheduler, six registers, fiber_main as the return address
    // (at a multiple of 16, so that fiber_main starts with the alignment of a called function), and a null return address that is never used
    uint64_t *top = (uint64_t *)(f->stack + STACK_BYTES);
    top[-1] = 0;
    top[-2] = (uint64_t)(uintptr_t)&fiber_main;
    for (int i = 3; i <= 8; ++i) top[-i] = 0;
    uint32_t *words = (uint32_t *)(top - 9);
    uint16_t fpcw;
    asm volatile("stmxcsr %0" : "=m"(words[0]));
    asm volatile("fnstcw %0" : "=m"(fpcw));
    words[1] = fpcw;
    f->ctx = (Context)(top - 9);
#else
    getcontext(&f->ctx);
    f->ctx.uc_stack.ss_sp = f->stack;
    f->ctx.uc_stack.ss_size = STACK_BYTES;
    f->ctx.uc_link = nullptr;
    makecontext(&f->ctx, fiber_main, 0);
#endif
}

Fiber *new_fiber()
{
    void *m = mmap(nullptr, STACK_BYTES + GUARD_BYTES, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (m == MAP_FAILED || mprotect(m, GUARD_BYTES, PROT_NONE) != 0) { fprintf(stderr, "emu: cannot map a fiber stack\n"); abort(); }
    Fiber *f = new Fiber;
    f->stack = (char *)m + GUARD_BYTES;
    return f;
}

uint64_t splitmix(uint64_t &x)
{
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// One workgroup, every thread of it.  Returns false when the fibers did not all meet at the same barriers.
bool run_group_threaded(dim3 block, int order, uint64_t seed, const std::function<void()> &body)
{
    Group &g = t_group;
    const unsigned n = block.x * block.y * block.z;
    while (g.fibers.size() < n) g.fibers.push_back(new_fiber());
    g.body = &body;
    std::vector<unsigned> turn(n);
    for (unsigned i = 0; i < n; ++i) turn[i] = order == THREADS_DESC ? n - 1 - i : i;
    if (order == THREADS_SEEDED)
        for (unsigned i = n; i > 1; --i) std::swap(turn[i - 1], turn[splitmix(seed) % i]);
    for (unsigned i = 0; i < n; ++i) {
        Fiber *f = g.fibers[i];
        start_at_fiber_main(f);
        f->done = false;
    }
    bool matched = true;
    for (unsigned live = n; live > 0;) {
        unsigned finished = 0;
        for (unsigned i = 0; i < n; ++i) {
            Fiber *f = g.fibers[turn[i]];
            if (f->done) continue;
            const unsigned t = turn[i];
            threadIdx = dim3(t % block.x, (t / block.x) % block.y, t / (block.x * block.y));
            resume(g, f);
            finished += f->done;
        }
        // some threads returned while others wait at a barrier (which is also how threads that pass different numbers of barriers end up)
        if (finished != 0 && finished != live) matched = false;
        live -= finished;
    }
    g.body = nullptr;
    return matched;
}

} // namespace

void __syncthreads()
{
    Group &g = t_group;
    Fiber *f = g.current;
    if (!f) return;                 // one thread per workgroup: it is alone at every barrier
    EMU_ASAN_START(&f->asan_fake, g.sched_stack, g.sched_size);
    switch_context(&f->ctx, &g.scheduler);
    EMU_ASAN_FINISH(f->asan_fake, &g.sched_stack, &g.sched_size);
}

void emu_launch(dim3 grid, dim3 block, size_t lds_bytes, const std::function<void()> &body)
{
    if (lds_bytes > 160 * 1024) { fprintf(stderr, "emu: LDS request %zu exceeds 160 KiB\n", lds_bytes); abort(); }
    const int order = g_thread_order.load(), threads = order & 3;
    const uint64_t seed = g_thread_seed.load();
    gridDim = grid;
    blockDim = threads == THREADS_ONE ? dim3(1, 1, 1) : block;
    threadIdx = dim3(0, 0, 0);
    const size_t groups = (size_t)grid.x * grid.y * grid.z;
    bool matched = true;
    for (size_t i = 0; i < groups; ++i) {
        const size_t id = (order & THREADS_GROUPS_DESC) ? groups - 1 - i : i;       // ascending: x fastest, as before
        blockIdx = dim3((unsigned)(id % grid.x), (unsigned)((id / grid.x) % grid.y), (unsigned)(id / ((size_t)grid.x * grid.y)));
        // poison LDS so that reads of unwritten slots are visible as garbage, not stale data
        memset(iopx::iopx_smem, 0xA5, lds_bytes);
        if (threads == THREADS_ONE) body();
        else matched = run_group_threaded(block, threads, seed ^ (0xD1B54A32D192ED03ull * (id + 1)), body) && matched;
    }
    if (!matched) ++g_barrier_mismatches;
}

namespace {

enum { SCHED_EAGER = 0, SCHED_ALL_LATE = 1, SCHED_ONE_LATE = 2 };
const int QUERY_BOUND = 64;             // not-ready answers one record gives before a query executes its stream (a loop that polls must end)
const unsigned char FRESH = 0xC7;       // what new device memory holds on a deferred schedule

struct Stream;
struct Marker { bool done = false; Stream *stream = nullptr; int queries = 0; };      // one hipEventRecord
struct Op {
    enum Kind { RUN, RECORD, WAIT } kind;
    std::function<void()> fn;
    std::shared_ptr<Marker> m;
};
struct Stream { std::deque<Op> q; int index = -1; };           // index: creation order among live created streams; -1: a handle from outside (0 = legacy)
struct Event { std::shared_ptr<Marker> last; };

struct State {
    std::recursive_mutex mu;
    std::map<hipStream_t, Stream *> streams;
    std::map<uintptr_t, size_t> pinned;                         // hipHostMalloc blocks: base -> bytes
    int late_index = -1;
    int drop_nth = -1, drop_stream = -1, waits_seen = 0;        // fault injection: see iopx_emu_drop_waits
    bool query_complete = false;
    int depth = 0;
};
State &st() { static State *s = new State; return *s; }        // never destroyed: the unload hook below still needs it
std::atomic<int> g_sched{ SCHED_EAGER };

Stream *lookup(hipStream_t h)
{
    State &S = st();
    auto it = S.streams.find(h);
    if (it == S.streams.end()) it = S.streams.emplace(h, new Stream).first;
    return it->second;
}

bool is_late(const Stream *s)
{
    const int sched = g_sched.load();
    return sched == SCHED_ALL_LATE || (sched == SCHED_ONE_LATE && s->index == st().late_index);
}

void run_until(Stream *s, const Marker *m);

void exec_front(Stream *s)
{
    Op op = std::move(s->q.front());
    s->q.pop_front();
    switch (op.kind) {
    case Op::RUN: op.fn(); break;
    case Op::RECORD: op.m->done = true; break;
    case Op::WAIT:
        if (!op.m->done) run_until(op.m->stream, op.m.get());
        if (!op.m->done) { fprintf(stderr, "emu: a stream waits for an event record that can never execute\n"); abort(); }
        break;
    }
}

// m = null: to the stream's end
void run_until(Stream *s, const Marker *m)
{
    State &S = st();
    if (++S.depth > 256) { fprintf(stderr, "emu: streams wait for each other in a cycle\n"); abort(); }
    while (!s->q.empty() && !(m && m->done)) exec_front(s);
    --S.depth;
}

void drain_all()
{
    State &S = st();
    for (bool again = true; again;) {
        again = false;
        for (auto &kv : S.streams) if (!kv.second->q.empty()) { run_until(kv.second, nullptr); again = true; }
    }
}

void enqueue(Stream *s, Op op)
{
    s->q.push_back(std::move(op));
    if (!is_late(s)) run_until(s, nullptr);
}

bool is_pinned(const void *p)
{
    State &S = st();
    auto it = S.pinned.upper_bound((uintptr_t)p);
    if (it == S.pinned.begin()) return false;
    --it;
    return (uintptr_t)p < it->first + it->second;
}

typedef std::lock_guard<std::recursive_mutex> Lock;

struct AtUnload { ~AtUnload() { Lock lk(st().mu); drain_all(); } } g_at_unload;

} // namespace

void emu_enqueue_launch(hipStream_t stream, dim3 grid, dim3 block, size_t lds_bytes, std::function<void()> body)
{
    if (g_sched.load() == SCHED_EAGER) { emu_launch(grid, block, lds_bytes, body); return; }
    Lock lk(st().mu);
    enqueue(lookup(stream), { Op::RUN, [grid, block, lds_bytes, body = std::move(body)]() { emu_launch(grid, block, lds_bytes, body); }, nullptr });
}

hipError_t hipSetDevice(int) { Lock lk(st().mu); drain_all(); return hipSuccess; }
hipError_t hipDeviceSynchronize() { Lock lk(st().mu); drain_all(); return hipSuccess; }

hipError_t hipStreamCreateWithFlags(hipStream_t *out, unsigned)
{
    State &S = st();
    Lock lk(S.mu);
    Stream *s = new Stream;
    for (s->index = 0;; ++s->index) {           // the lowest creation index no live stream holds
        bool taken = false;
        for (auto &kv : S.streams) taken = taken || kv.second->index == s->index;
        if (!taken) break;
    }
    S.streams[(hipStream_t)s] = s;
    *out = (hipStream_t)s;
    return hipSuccess;
}

hipError_t hipStreamDestroy(hipStream_t h)
{
    State &S = st();
    Lock lk(S.mu);
    auto it = S.streams.find(h);
    if (it == S.streams.end()) return hipSuccess;
    run_until(it->second, nullptr);
    delete it->second;
    S.streams.erase(it);
    return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t h)
{
    if (g_sched.load() == SCHED_EAGER) return hipSuccess;
    Lock lk(st().mu);
    run_until(lookup(h), nullptr);
    return hipSuccess;
}

hipError_t hipMalloc(void **p, size_t n)
{
    *p = malloc(n ? n : 8);
    if (!*p) return hipErrorUnknown;
    if (g_sched.load() != SCHED_EAGER) memset(*p, FRESH, n ? n : 8);     // a read of never-written memory gives the same wrong bytes every run
    return hipSuccess;
}
hipError_t hipFree(void *p) { { Lock lk(st().mu); drain_all(); } free(p); return hipSuccess; }
hipError_t hipMallocAsync(void **p, size_t n, hipStream_t) { return hipMalloc(p, n); }
hipError_t hipFreeAsync(void *p, hipStream_t) { return hipFree(p); }

hipError_t hipHostMalloc(void **p, size_t n, unsigned)
{
    *p = malloc(n ? n : 8);
    if (!*p) return hipErrorUnknown;
    Lock lk(st().mu);
    st().pinned[(uintptr_t)*p] = n ? n : 8;
    return hipSuccess;
}
hipError_t hipHostFree(void *p)
{
    { Lock lk(st().mu); drain_all(); st().pinned.erase((uintptr_t)p); }
    free(p);
    return hipSuccess;
}

// As the real runtime: a copy to or from pinned host memory is queued and touches that memory when it executes; a pageable source is
// staged at the call; a pageable destination makes the call wait for the stream and copy then.
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind kind, hipStream_t stream)
{
    if (g_sched.load() == SCHED_EAGER) { memmove(d, s, n); return hipSuccess; }
    Lock lk(st().mu);
    Stream *q = lookup(stream);
    if (kind == hipMemcpyDeviceToDevice || (kind == hipMemcpyHostToDevice && is_pinned(s)) || (kind == hipMemcpyDeviceToHost && is_pinned(d))) {
        enqueue(q, { Op::RUN, [d, s, n]() { memmove(d, s, n); }, nullptr });
    } else if (kind == hipMemcpyHostToDevice) {
        auto staged = std::make_shared<std::vector<unsigned char>>((const unsigned char *)s, (const unsigned char *)s + n);
        enqueue(q, { Op::RUN, [d, staged, n]() { memcpy(d, staged->data(), n); }, nullptr });
    } else {
        run_until(q, nullptr);
        memmove(d, s, n);
    }
    return hipSuccess;
}

hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t stream)
{
    if (g_sched.load() == SCHED_EAGER) { memset(d, v, n); return hipSuccess; }
    Lock lk(st().mu);
    enqueue(lookup(stream), { Op::RUN, [d, v, n]() { memset(d, v, n); }, nullptr });
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t) new Event; return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) { Lock lk(st().mu); delete (Event *)e; return hipSuccess; }      // queued records and waits hold their Marker

hipError_t hipEventRecord(hipEvent_t e, hipStream_t stream)
{
    if (!e) return hipErrorUnknown;
    Lock lk(st().mu);
    Stream *s = lookup(stream);
    auto m = std::make_shared<Marker>();
    m->stream = s;
    ((Event *)e)->last = m;
    enqueue(s, { Op::RECORD, nullptr, m });
    return hipSuccess;
}

// waits for the record that is the event's most recent one NOW; an event never recorded holds nothing back
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t e, unsigned)
{
    if (!e) return hipErrorUnknown;
    State &S = st();
    Lock lk(S.mu);
    Stream *s = lookup(stream);
    if (S.drop_nth >= 0 && (S.drop_stream < 0 || S.drop_stream == s->index)) {
        ++S.waits_seen;
        if (S.drop_nth == 0 || S.drop_nth == S.waits_seen) return hipSuccess;       // injected fault: the edge is lost
    }
    std::shared_ptr<Marker> m = ((Event *)e)->last;
    if (m && !m->done) enqueue(s, { Op::WAIT, nullptr, m });
    return hipSuccess;
}

static hipError_t marker_ready(const std::shared_ptr<Marker> &m, bool poll)
{
    if (!m || m->done || st().query_complete) return hipSuccess;
    if (poll && ++m->queries > QUERY_BOUND) { run_until(m->stream, m.get()); return hipSuccess; }
    return hipErrorNotReady;            // a query makes no progress by itself
}

hipError_t hipEventQuery(hipEvent_t e)
{
    if (!e) return hipErrorUnknown;
    Lock lk(st().mu);
    return marker_ready(((Event *)e)->last, true);
}

hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b)
{
    *ms = 0.f;
    if (!a || !b) return hipErrorUnknown;
    Lock lk(st().mu);
    const hipError_t ea = marker_ready(((Event *)a)->last, false), eb = marker_ready(((Event *)b)->last, false);
    return ea != hipSuccess ? ea : eb;
}

// ---- test-only entries -------------------------------------------------------------------------------------------------------------
static void k_emu_set(uint64_t *p, uint64_t v) { if (blockIdx.x == 0) *p = v; }
static void k_emu_copy(uint64_t *d, const uint64_t *s) { if (blockIdx.x == 0) *d = *s; }

extern "C" {

// schedule: 0 eager, 1 all streams late, 2 the stream with creation index `late_stream` late.  Drains everything first.
int iopx_emu_set_schedule(int schedule, int late_stream)
{
    if (schedule < SCHED_EAGER || schedule > SCHED_ONE_LATE) return -1;
    Lock lk(st().mu);
    drain_all();
    st().late_index = late_stream;
    g_sched.store(schedule);
    return 0;
}

// Thread order of every launch from now on (see the threaded mode above); returns the order that held before, or -1 for an order that does not
// exist.  Drains everything first, so a launch already queued runs under the order that held when it was made.
int iopx_emu_set_threads(int order, uint64_t seed)
{
    if (order < 0 || order > 7) return -1;
    Lock lk(st().mu);
    drain_all();
    g_thread_seed.store(seed);
    return g_thread_order.exchange(order);
}

// launches since the last call in which the threads of some workgroup did not all meet at the same barriers; clears the count
long iopx_emu_barrier_mismatches(void)
{
    Lock lk(st().mu);
    drain_all();
    return g_barrier_mismatches.exchange(0);
}

// created streams alive (the library's own is the first, its side stream the second)
int iopx_emu_live_streams(void)
{
    Lock lk(st().mu);
    int n = 0;
    for (auto &kv : st().streams) n += kv.second->index >= 0;
    return n;
}

// Fault injection.  nth < 0: off; 0: every hipStreamWaitEvent from now on is a no-op; n > 0: the n-th one from now on.  on_stream >= 0: only
// waits enqueued on the stream with that creation index are counted and dropped.
void iopx_emu_drop_waits(int nth, int on_stream)
{
    Lock lk(st().mu);
    st().drop_nth = nth; st().drop_stream = on_stream; st().waits_seen = 0;
}

// Fault injection: hipEventQuery and hipEventElapsedTime report completion whatever the record's state
void iopx_emu_force_query_complete(int on)
{
    Lock lk(st().mu);
    st().query_complete = on != 0;
}

// The scheduler's self-tests, written against the fake API alone.  Each returns what it observed, packed in decimal digits; the expected
// value per schedule is in tests/stream_schedule_cases.py.  Device memory is host memory here, so a test may look at it without a copy.
long iopx_emu_selftest(int which)
{
    hipStream_t A = nullptr, B = nullptr;
    hipEvent_t e = nullptr;
    uint64_t *x = nullptr, *y = nullptr, *z = nullptr, *pin = nullptr, *spare = nullptr;
    uint64_t *page = (uint64_t *)malloc(8);
    (void)hipStreamCreateWithFlags(&A, hipStreamNonBlocking);
    (void)hipStreamCreateWithFlags(&B, hipStreamNonBlocking);
    (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    (void)hipMalloc(&x, 8); (void)hipMalloc(&y, 8); (void)hipMalloc(&z, 8); (void)hipMalloc(&spare, 8);
    (void)hipHostMalloc((void **)&pin, 8, 0);
    hipLaunchKernelGGL(k_emu_set, dim3(2), dim3(64), 0, A, x, 1);
    hipLaunchKernelGGL(k_emu_set, dim3(2), dim3(64), 0, A, y, 2);
    hipLaunchKernelGGL(k_emu_set, dim3(2), dim3(64), 0, A, z, 3);
    (void)hipStreamSynchronize(A);
    long r = -1;
    switch (which) {
    case 0: case 1: {           // A writes x, B reads it into y: without (0) and with (1) an event between them.  Returns y.
        uint64_t v = 5;
        hipLaunchKernelGGL(k_emu_set, dim3(2), dim3(64), 0, A, x, v);
        v = 6;                  // the launch took its copy
        if (which == 1) { (void)hipEventRecord(e, A); (void)hipStreamWaitEvent(B, e, 0); }
        hipLaunchKernelGGL(k_emu_copy, dim3(1), dim3(64), 0, B, y, x);
        (void)hipStreamSynchronize(B);
        (void)hipStreamSynchronize(A);
        r = (long)*y;
        break;
    }
    case 2: {                   // a wait holds the record current at the call, and pulls the other stream up to it and no further.  Returns y * 100 + x.
        hipLaunchKernelGGL(k_emu_set, dim3(1), dim3(64), 0, A, x, 5);
        (void)hipEventRecord(e, A);
        (void)hipStreamWaitEvent(B, e, 0);
        hipLaunchKernelGGL(k_emu_copy, dim3(1), dim3(64), 0, B, y, x);
        hipLaunchKernelGGL(k_emu_set, dim3(1), dim3(64), 0, A, x, 7);
        (void)hipEventRecord(e, A);
        (void)hipStreamSynchronize(B);
        r = (long)*y * 100 + (long)*x;
        break;
    }
    case 3: {                   // hipStreamSynchronize(B) leaves A's work pending.  Returns x before A is synchronised * 10000 + z * 100 + x after.
        hipLaunchKernelGGL(k_emu_set, dim3(1), dim3(64), 0, A, x, 5);
        hipLaunchKernelGGL(k_emu_set, dim3(1), dim3(64), 0, B, z, 9);
        (void)hipStreamSynchronize(B);
        r = (long)*x * 10000 + (long)*z * 100;
        (void)hipStreamSynchronize(A);
        r += (long)*x;
        break;
    }
    case 4: {                   // host memory in asynchronous copies.  Returns (pageable read-back, seen at once) * 100 + (x from pinned) * 10 + (z from pageable).
        *pin = 1; *page = 1;
        (void)hipMemcpyAsync(x, pin, 8, hipMemcpyHostToDevice, A);
        (void)hipMemcpyAsync(z, page, 8, hipMemcpyHostToDevice, A);
        *pin = 2; *page = 2;
        (void)hipStreamSynchronize(A);
        r = (long)*x * 10 + (long)*z;
        hipLaunchKernelGGL(k_emu_set, dim3(1), dim3(64), 0, A, y, 5);
        (void)hipMemcpyAsync(page, y, 8, hipMemcpyDeviceToHost, A);
        r += (long)*page * 100;
        break;
    }
    case 5: {                   // hipFree drains every stream.  Returns x * 10 + z right after the call.
        hipLaunchKernelGGL(k_emu_set, dim3(1), dim3(64), 0, A, x, 5);
        hipLaunchKernelGGL(k_emu_set, dim3(1), dim3(64), 0, B, z, 9);
        (void)hipFree(spare);
        spare = nullptr;
        r = (long)*x * 10 + (long)*z;
        break;
    }
    case 6: {                   // queries: not ready while the record is pending, no progress by a few of them, and a polling loop ends.
        hipLaunchKernelGGL(k_emu_set, dim3(1), dim3(64), 0, A, x, 5);    // Returns (first answer not ready) * 1000000 + x after 3 queries * 100000 + polls needed * 100 + x at the end
        (void)hipEventRecord(e, A);
        const bool pending = hipEventQuery(e) == hipErrorNotReady;
        (void)hipEventQuery(e); (void)hipEventQuery(e);
        r = (pending ? 1000000 : 0) + (long)*x * 100000;
        int polls = 0;
        while (hipEventQuery(e) != hipSuccess && polls < 999) ++polls;
        r += polls * 100 + (long)*x;
        break;
    }
    default: break;
    }
    (void)hipStreamSynchronize(A);
    (void)hipStreamSynchronize(B);
    (void)hipEventDestroy(e);
    (void)hipStreamDestroy(A);
    (void)hipStreamDestroy(B);
    (void)hipFree(x); (void)hipFree(y); (void)hipFree(z);
    if (spare) (void)hipFree(spare);
    (void)hipHostFree(pin);
    free(page);
    return r;
}

} // extern "C"
