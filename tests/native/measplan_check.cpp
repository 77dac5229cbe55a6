// Stand-alone check of rsp_measplan.h (tests/test_measplan_cpu.py): the hit-list geometry of
// hand-worked shapes -- the rows of tests/measure_cases.py and the values of R either side of
// every threshold.  Prints "ok" or the failures.
#include <cstdint>
#include <cstdio>

#include "rsp_measplan.h"

static int g_bad = 0;

struct Want {
    const char* id;
    int64_t V, R, ld, cs;
    uintptr_t addr;
    bool wide;
    int G, S, rows, q, passes;
};

static void check(const Want& w) {
    const rsp::MeasPlan p = rsp::meas_plan(w.V, w.R, w.ld, w.cs, w.addr, 1);
    const bool ok = p.wide == w.wide && p.cw == (w.wide ? 16 : 1) && p.G == w.G && p.S == w.S && p.rows == w.rows &&
                    p.q == w.q && p.passes == w.passes && p.bands == 1;
    if (!ok) {
        ++g_bad;
        std::fprintf(stderr, "%s: got wide %d cw %d G %d S %d rows %d q %d passes %d bands %d\n", w.id, (int)p.wide, p.cw,
                     p.G, p.S, p.rows, p.q, p.passes, p.bands);
    }
    // what the kernel relies on: the slices cover V, the passes cover R, the mask has a bit per q rows
    if ((int64_t)p.S * p.rows < w.V || (int64_t)p.passes * p.G * p.cw < w.R || p.G * p.S != rsp::kMeasThreads ||
        (int64_t)(p.passes - 1) * p.G * p.cw >= w.R || (p.rows + p.q - 1) / p.q > 64) {
        ++g_bad;
        std::fprintf(stderr, "%s: the plan does not cover %lld x %lld\n", w.id, (long long)w.V, (long long)w.R);
    }
}

int main() {
    const uintptr_t A = 0x7f0000001000u;   // a 16-byte aligned address
    const Want table[] = {
        // the case table: id, V, R, ld, cs, address, wide, G, S, rows, q, passes
        {"w-min", 8, 256, 256, 8 * 256, A, true, 16, 64, 1, 1, 1},                 // 16 groups; 56 empty slices
        {"w-ragged", 130, 256, 256, 130 * 256, A, true, 16, 64, 3, 1, 1},          // 43 * 3 = 129: slice 43 has 1 row
        {"w-q2", 261, 4096, 4096, 261 * 4096, A, true, 256, 4, 66, 2, 1},          // 256 groups; ceil(261/4) = 66 > 64
        {"w-2pass", 8, 16400, 16400, 8 * 16400, A, true, 1024, 1, 8, 1, 2},        // 1025 groups: 1024 + 1
        {"w-window", 40, 256, 304, 40 * 304 + 32, A + 16, true, 16, 64, 1, 1, 1},  // column 16 of ld 304
        {"b-col7", 40, 256, 304, 40 * 304 + 32, A + 7, false, 256, 4, 10, 1, 1},   // the address alone
        {"b-ld", 40, 256, 300, 40 * 300, A, false, 256, 4, 10, 1, 1},              // the pitch alone
        {"b-cs", 40, 256, 256, 40 * 256 + 8, A, false, 256, 4, 10, 1, 1},          // the CPI stride alone
        {"b-240", 40, 240, 240, 40 * 240, A, false, 256, 4, 10, 1, 1},             // 15 groups of 16: too few
        {"b-2pass", 8, 1030, 1030, 8 * 1030, A, false, 1024, 1, 8, 1, 2},          // 1024 + 6 columns
        {"b-3pass", 8, 2055, 2055, 8 * 2055, A, false, 1024, 1, 8, 1, 3},          // 1024 + 1024 + 7
        {"b-1025", 12, 1025, 1025, 12 * 1025, A, false, 1024, 1, 12, 1, 2},        // 1024 + 1
        {"tight-1", 4, 3, 3, 12, A, false, 64, 16, 1, 1, 1},
        {"tight-4", 16, 9, 9, 144, A, false, 64, 16, 1, 1, 1},
        {"interp", 48, 300, 300, 48 * 300, A, false, 512, 2, 24, 1, 1},
        {"e-all", 64, 272, 272, 64 * 272, A, true, 32, 32, 2, 1, 1},               // 17 groups -> 32
        // R either side of the thresholds
        {"R255", 64, 255, 255, 64 * 255, A, false, 256, 4, 16, 1, 1},
        {"R256", 64, 256, 256, 64 * 256, A, true, 16, 64, 1, 1, 1},
        {"R272", 64, 272, 272, 64 * 272, A, true, 32, 32, 2, 1, 1},
        {"R1024", 64, 1024, 1024, 64 * 1024, A, true, 64, 16, 4, 1, 1},
        {"R1024b", 64, 1024, 1024, 64 * 1024, A + 1, false, 1024, 1, 64, 1, 1},    // bytes: exactly one pass
        {"R1025", 64, 1025, 1025, 64 * 1025, A, false, 1024, 1, 64, 1, 2},
        {"R16384", 8, 16384, 16384, 8 * 16384, A, true, 1024, 1, 8, 1, 1},         // wide: exactly one pass
        {"R16400", 8, 16400, 16400, 8 * 16400, A, true, 1024, 1, 8, 1, 2},
        // shapes of the existing suite
        {"8192", 32, 8192, 8192, 32 * 8192, A, true, 512, 2, 16, 1, 1},            // one pass, not several
        {"dmx-short", 2048, 62, 574, 2048 * 574, A, false, 64, 16, 128, 2, 1},
        {"dmx-long", 2048, 512, 574, 2048 * 574, A + 62, false, 512, 2, 1024, 16, 1},
        {"65rows", 65, 16384, 16384, 65 * 16384, A, true, 1024, 1, 65, 2, 1},      // q steps at 64 rows
    };
    for (const Want& w : table) check(w);
    // bands: the rows of a slice are those of one band
    const rsp::MeasPlan b = rsp::meas_plan(2048, 512, 512, 2048 * 512, A, 4);
    if (!(b.wide && b.G == 32 && b.S == 32 && b.bands == 4 && b.rows == 16 && b.q == 1 && b.passes == 1)) {
        ++g_bad;
        std::fprintf(stderr, "bands 4: rows %d q %d\n", b.rows, b.q);
    }
    if (rsp::meas_plan(8, 256, 256, 2048, A, 0).bands != 1) {
        ++g_bad;
        std::fprintf(stderr, "bands 0 is one band\n");
    }
    if (g_bad == 0) std::puts("ok");
    return g_bad ? 1 : 0;
}
