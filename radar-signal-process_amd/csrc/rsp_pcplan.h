// rsp_pcplan.h -- how a pulse-compression launch's units are dealt to its workgroups.
// Pure host code (no HIP), so a stand-alone program can test it: tests/native/pcplan_check.cpp.
//
// A unit is a (row, overlap-save sub-block) pair.  A workgroup holds `rpb` rows side by side
// (PairCfg::RPB1 / RPB2) and, on the multi-row path of the 4096-point rows, each of them walks
// `rows` consecutive units: workgroup b, row slot g starts at unit (b * rpb + g) * rows.  Units
// past the end run as invalid rows (no loads, no stores), so the count only has to cover them.
#pragma once
#include <cstdint>

namespace rsp {

// rows per workgroup slot the library uses when rsp_set_pc_rows was not called (or was given 0):
// 2 won the c3 A/B and is not slower than 1 at c2, c4 and c5
constexpr int kPcRowsDefault = 2;

inline bool pc_rows_valid(int n) { return n == 1 || n == 2 || n == 4; }

inline int pc_blocks(int64_t units, int rpb, int rows) {
    if (units <= 0 || rpb < 1 || rows < 1) return 0;
    const int64_t per = (int64_t)rpb * rows;
    return (int)((units + per - 1) / per);
}

}  // namespace rsp
