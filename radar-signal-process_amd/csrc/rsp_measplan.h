// rsp_measplan.h -- the geometry of a hit-list launch (hits_kernel and the band kernels of
// rsp_measure.hip): which flag-load path a call takes and how one CPI's columns and rows are
// dealt to the 1024 threads of a workgroup.  Pure host code (no HIP), so a stand-alone program
// can test it: tests/native/measplan_check.cpp.  launch_e and launch_hit_list take every one of
// these numbers from here, and rsp_measure_plan reports them.  (The kernels are handed G and
// derive S, rows and q from it and V by the expressions below.)
//
// A thread owns `cw` adjacent columns (16: one 16-byte flag load per row; 1: one byte) of one
// of S row slices.  A pass covers G * cw columns; `passes` passes cover R.  Slice s owns rows
// min(V, s * rows) .. min(V, s * rows + rows), so with V < S the later slices are empty and with
// S not dividing V the last used one is short.  A thread keeps one mask bit per q of its rows.
#pragma once
#include <cstdint>

namespace rsp {

constexpr int kMeasThreads = 1024;   // threads of a hit-list workgroup

struct MeasPlan {
    bool wide;    // 16-byte flag loads
    int cw;       // columns per thread: 16 (wide) or 1
    int G;        // column groups per pass: a power of two, 16 (wide) / 64 (bytes) .. 1024
    int S;        // row slices: 1024 / G
    int rows;     // rows per slice: ceil(Vb / S), Vb = V (one band) or ceil(V / bands)
    int q;        // rows per bit of a thread's 64-bit row mask: ceil(rows / 64)
    int passes;   // column passes: ceil(R / (G * cw))
    int bands;    // workgroups per CPI (1: hits_kernel)
};

// flag_addr: the address of the first CPI's first flag byte (only its low four bits matter).
// The 16-byte path needs every row of every CPI 16-byte aligned (the address, the pitch and the
// CPI stride), whole 16-column groups (R % 16 == 0) and at least 16 of them.
inline MeasPlan meas_plan(int64_t V, int64_t R, int64_t ld, int64_t cs, uintptr_t flag_addr, int bands) {
    MeasPlan p{};
    p.wide = R % 16 == 0 && R >= 16 * 16 && ld % 16 == 0 && cs % 16 == 0 && (flag_addr & 15) == 0;
    p.cw = p.wide ? 16 : 1;
    // column groups per pass: a power of two covering the columns (16-byte groups: at least 16,
    // one 256-byte row segment per 16 lanes; bytes: at least 64), at most 1024
    int G = p.wide ? 16 : 64;
    const int64_t groups = p.wide ? R / 16 : R;
    while (G < groups && G < kMeasThreads) G <<= 1;
    p.G = G;
    p.S = kMeasThreads / G;
    p.bands = bands < 1 ? 1 : bands;
    const int64_t Vb = (V + p.bands - 1) / p.bands;
    p.rows = (int)((Vb + p.S - 1) / p.S);
    p.q = (p.rows + 63) / 64;
    const int64_t per = (int64_t)G * p.cw;
    p.passes = (int)((R + per - 1) / per);
    return p;
}

}  // namespace rsp
