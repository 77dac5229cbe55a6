// rsp_chunkplan.h -- how a chain call's units are cut into chunks and dealt to the pipelines.
// Pure host code (no HIP), so a stand-alone program can test it: tests/native/chunkplan_check.cpp.
//
// Chunk k runs on lane k % ns.  Every lane has its own steady-state chunk size cu[lane], so the
// stream is cut cu[0], cu[1], ..., cu[ns-1], cu[0], ... and only the final chunk is short.  With
// unequal sizes the lanes have unequal periods, so their PC / MTD phases drift against each other
// instead of locking.  Everything a lane's buffers are sized by -- PC scratch and
// concat slots, RDM slots, hit-list regions -- must use the lane's or the plan's fixed capacity,
// never the current chunk's size: a short last chunk on lane 1 must not land inside lane 0's slot.
#pragma once
#include <cstdint>
#include <vector>

namespace rsp {

constexpr int kMaxLanes = 4;

struct ChunkPlan {
    std::vector<int64_t> cstart;     // chunk k covers units [cstart[k], cstart[k + 1])
    int ns = 0;                      // lanes in use: min(lanes asked for, chunks)
    int64_t cap[kMaxLanes] = {};     // lane's largest chunk (units); 0 for an unused lane
    int64_t cap_max = 0;             // the largest chunk of the call: sizes every per-lane slot
    int64_t period = 0;              // units of one round over the lanes (sum of cap)
    int64_t nchunks() const { return (int64_t)cstart.size() - 1; }
    int lane(int64_t k) const { return (int)(k % ns); }
    int64_t on_lane(int64_t k) const { return k / ns; }   // the chunk's index on its lane
};

// units > 0; cu[0..nlanes) >= 1 each (clamped to units); nlanes in 1..kMaxLanes.
inline ChunkPlan plan_chunks(int64_t units, const int64_t* cu, int nlanes) {
    ChunkPlan p;
    p.cstart.push_back(0);
    if (units <= 0 || nlanes < 1) return p;
    if (nlanes > kMaxLanes) nlanes = kMaxLanes;
    for (int64_t k = 0; p.cstart.back() < units; ++k) {
        int64_t c = cu[k % nlanes];
        if (c < 1) c = 1;
        const int64_t e = p.cstart.back() + c;
        p.cstart.push_back(e < units ? e : units);
    }
    const int64_t n = p.nchunks();
    p.ns = (int)(n < nlanes ? n : nlanes);
    for (int64_t k = 0; k < n; ++k) {
        const int64_t len = p.cstart[(size_t)k + 1] - p.cstart[(size_t)k];
        int64_t& c = p.cap[p.lane(k)];
        if (len > c) c = len;
    }
    for (int l = 0; l < p.ns; ++l) {
        p.period += p.cap[l];
        if (p.cap[l] > p.cap_max) p.cap_max = p.cap[l];
    }
    return p;
}

// The default two-lane split of an unset chunk (equal chunks of `cu` units otherwise): lanes of
// a and b units, used only when the batch holds at least kLaneRounds rounds of both, so short
// calls keep the equal plan they always had.
constexpr int kLaneRounds = 4;
inline bool lane_split_applies(int64_t units, int64_t a, int64_t b) {
    return a >= 1 && b >= 1 && a != b && units >= kLaneRounds * (a + b);
}

}  // namespace rsp
