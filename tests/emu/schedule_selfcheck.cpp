// TEST INFRASTRUCTURE ONLY — a stand-alone program for the sanitizer build of the emulation (make -C tests/emu schedule_selfcheck_san):
// the scheduler's self-tests on the eager and the all-late schedule, then one small Aurora proof over gf192 through the C ABI on both, which
// must give the same bytes.  Queued closures are where lifetimes go wrong (an argument that points into a dead host frame); nothing here is
// loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../../include/libiop_amd.h"

extern "C" {
int iopx_emu_set_schedule(int schedule, int late_stream);
int iopx_emu_live_streams(void);
long iopx_emu_selftest(int which);
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
    expect(iopx_clear_plans() == IOPX_OK, "iopx_clear_plans", 0);          // the pool's blocks and the plan caches go back: what is left at exit is a leak
    if (failures == 0) printf("schedule_selfcheck: ok (%zu transcript bytes)\n", reference.size());
    return failures ? 1 : 0;
}
