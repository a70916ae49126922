// TEST INFRASTRUCTURE ONLY — a stand-alone program for the sanitizer build of the emulation (make -C tests/emu schedule_selfcheck_san):
// the scheduler's self-tests on the eager and the all-late schedule, then one small Aurora proof over gf192 through the C ABI on both, which
// must give the same bytes.  Queued closures are where lifetimes go wrong (an argument that points into a dead host frame); nothing here is
// loaded into Python.  Then the threaded mode: a toy kernel and one gf192 transform with one fiber per thread, so that the fiber stacks and the
// context switches (ucontext in this build, with the sanitizer told of every switch) run under both sanitizers once.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/libiop_amd.h"

extern "C" {
int iopx_emu_set_schedule(int schedule, int late_stream);
int iopx_emu_live_streams(void);
long iopx_emu_selftest(int which);
int iopx_emu_set_threads(int order, uint64_t seed);
long iopx_emu_barrier_mismatches(void);
int iopx_emu_toy(int which, int barrier, int n, uint64_t *out);
}

// The library keeps its pinned staging chunks, with one event each, for the life of the process (runtime.hip, upload): not leaks.  Everything
// else still alive at exit is reported.
extern "C" const char *__lsan_default_suppressions() { return "leak:iopx::upload\n"; }

static int failures = 0;
static void expect(bool ok, const char *what, long got)
{
    if (!ok) { fprintf(stderr, "FAILED: %s (got %ld)\n", what, got); ++failures; }
}

static std::string prove(iopx_aurora_instance *inst)
{
    uint8_t *t = nullptr;
    size_t n = 0;
    if (iopx_aurora_prove(inst, 128, 5, 2, &t, &n) != IOPX_OK) { fprintf(stderr, "FAILED: iopx_aurora_prove: %s\n", iopx_last_error()); ++failures; return ""; }
    std::string out((const char *)t, n);
    iopx_host_free(t);
    return out;
}

// the threaded mode: descending thread index, workgroups in descending order (order 2 | 4)
static void threaded_mode()
{
    const int n = 128;
    std::vector<uint64_t> out(n);
    expect(iopx_emu_set_threads(2 | 4, 1) == 0, "the default order is one thread per workgroup", 0);
    expect(iopx_emu_toy(1, 1, n, out.data()) == 0, "toy kernel", 0);
    bool right = true;
    for (int i = 0; i < n; ++i) right = right && out[i] == 0x1000 + 7 * (uint64_t)(i > 0 ? i - 1 : 0);
    expect(right, "with its barrier the toy kernel reads its neighbour's slot", 0);
    expect(iopx_emu_barrier_mismatches() == 0, "barrier discipline of the toy kernel", 0);
    expect(iopx_emu_toy(5, 1, n, out.data()) == 0 && iopx_emu_barrier_mismatches() == 1, "a skipped barrier is counted", 0);
    iopx_emu_set_threads(0, 0);

    // 2^12 coefficients over gf192: phase 1, a five-level and a one-level comb tile, the edge pass
    const int m = 12;
    std::vector<uint64_t> coeffs(3 << m), basis(3 * m, 0), shift = { 5, 0, 1 }, one(3 << m), many(3 << m), back(3 << m);
    uint64_t x = 0x2204;
    for (auto &w : coeffs) { x = x * 6364136223846793005ull + 1442695040888963407ull; w = x; }
    for (int i = 0; i < m; ++i) basis[3 * i] = 1ull << i;
    expect(iopx_add_fft_gf192(coeffs.data(), (size_t)1 << m, basis.data(), m, shift.data(), one.data()) == IOPX_OK, "transform, one thread per workgroup", 0);
    iopx_emu_set_threads(2 | 4, 1);
    expect(iopx_add_fft_gf192(coeffs.data(), (size_t)1 << m, basis.data(), m, shift.data(), many.data()) == IOPX_OK, "transform, threaded", 0);
    expect(iopx_add_ifft_gf192(many.data(), basis.data(), m, shift.data(), back.data()) == IOPX_OK, "inverse transform, threaded", 0);
    expect(iopx_emu_barrier_mismatches() == 0, "barrier discipline of the transform", 0);
    iopx_emu_set_threads(0, 0);
    expect(many == one, "the threaded transform equals the one-thread one", 0);
    expect(back == coeffs, "the threaded inverse gives the coefficients back", 0);
}

int main()
{
    if (iopx_init(0) != IOPX_OK) { fprintf(stderr, "iopx_init: %s\n", iopx_last_error()); return 2; }
    if (iopx_side_stream_begin() != IOPX_OK || iopx_side_stream_end() != IOPX_OK || iopx_side_stream_join() != IOPX_OK) return 2;
    expect(iopx_emu_live_streams() == 2, "the library's own stream and its side stream", iopx_emu_live_streams());

    static const long eager[7] = { 5, 5, 507, 50905, 511, 59, 500005 }, late[7] = { 1, 5, 505, 10905, 521, 59, 1106105 };
    for (int which = 0; which < 7; ++which) expect(iopx_emu_selftest(which) == eager[which], "self-test, eager", which);
    iopx_emu_set_schedule(1, -1);
    for (int which = 0; which < 7; ++which) expect(iopx_emu_selftest(which) == late[which], "self-test, all streams late", which);
    iopx_emu_set_schedule(0, -1);

    iopx_aurora_instance *inst = nullptr;
    if (iopx_aurora_example_instance_create(IOPX_FIELD_GF192, 64, 7, 63, 0x2204, &inst) != IOPX_OK) { fprintf(stderr, "instance: %s\n", iopx_last_error()); return 2; }
    const std::string reference = prove(inst);
    iopx_emu_set_schedule(1, -1);
    const std::string first = prove(inst), second = prove(inst);
    iopx_emu_set_schedule(0, -1);
    expect(!reference.empty() && first == reference, "the first all-late proof equals the eager one", (long)first.size());
    expect(second == reference, "the second all-late proof equals the eager one", (long)second.size());
    iopx_aurora_instance_free(inst);
    threaded_mode();
    expect(iopx_clear_plans() == IOPX_OK, "iopx_clear_plans", 0);          // the pool's blocks and the plan caches go back: what is left at exit is a leak
    if (failures == 0) printf("schedule_selfcheck: ok (%zu transcript bytes)\n", reference.size());
    return failures ? 1 : 0;
}
