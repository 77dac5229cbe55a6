// rsp_cfar_dev.h -- the CFAR building blocks that both the MTD kernels (rsp_mtd.hip) and the
// CFAR kernels (rsp_cfar.hip) inline (device code only).
#pragma once
#include <hip/hip_runtime.h>

#include "rsp_buf.h"
#include "rsp_internal.h"

namespace rsp {

// ================================================================== CFAR building blocks
// Reference windows of Function_CFAR1D_sub.m:25-28 around cell y of a line whose valid
// part is [lo, hi): left = [y-save-ref, y-save-1], right = [y+save+1, y+save+ref]; a side
// that leaves [lo, hi) is replaced by the other side's mean (:30-39).  Window sums are
// precomputed as direct left-to-right sums of `ref` cells (the order mean() adds them),
// so a cell needs two sum lookups.  max/min of the two means = max/min of the two sums
// divided once (division by a positive constant is monotonic in IEEE arithmetic).
__device__ __forceinline__ uint8_t cfar_test(float x, float sl, float sr, bool lok, bool rok, int method, float Tr) {
    // fp32 threshold max|min(sum_L, sum_R) * (T/ref); the fp64 reference computes
    // (sum/ref)*T -- the two differ by ~1 ulp, far inside the near-threshold band
    const float a = lok ? sl : sr;
    const float b = rok ? sr : sl;
    return x >= (method == 0 ? fmaxf(a, b) : fminf(a, b)) * Tr ? 1 : 0;
}

__device__ __forceinline__ bool in_segs(int c, int nseg, const int* lo, const int* hi) {
    bool in = false;
#pragma unroll
    for (int s = 0; s < RSP_MAX_SEG; ++s)
        if (s < nseg) in |= (c >= lo[s] && c < hi[s]);
    return in;
}

__device__ __forceinline__ void seg_of(int c, int nseg, const int* lo, const int* hi, int& slo, int& shi) {
    slo = 0;
    shi = 0;
#pragma unroll
    for (int s = 0; s < RSP_MAX_SEG; ++s)
        if (s < nseg && c >= lo[s] && c < hi[s]) {
            slo = lo[s];
            shi = hi[s];
        }
}

// Doppler CFAR over a column-major tile in LDS: column c = mag[c*ms + v], v < V (zero band
// already applied).  Thread (c, g) owns rows [v0, v1); sums[c*ms + a] must hold the window
// sums for every a with a + ref <= V.  Writes flags to out[v*R] (out already offset by r).
__device__ __forceinline__ void doppler_sums(const float* mag, float* sums, int V, int ref, int v0, int v1) {
    for (int a = v0; a < v1; ++a) {
        if (a + ref > V) break;
        float s = 0.f;
        for (int k = 0; k < ref; ++k) s += mag[a + k];
        sums[a] = s;
    }
}

__device__ __forceinline__ uint8_t doppler_test(const float* mag, const float* sums, const CfarVArgs& cv,
                                                bool col_on, int v) {
    uint8_t f = 0;
    if (col_on && v >= cv.lo && v < cv.hi) {
        const int l1 = v - cv.save - cv.ref, r1 = v + cv.save + 1;
        const bool lok = l1 >= cv.lo, rok = r1 + cv.ref <= cv.hi;
        f = cfar_test(mag[v], lok ? sums[l1] : 0.f, rok ? sums[r1] : 0.f, lok, rok, cv.method, cv.Tr);
    }
    return f;
}

__device__ __forceinline__ void doppler_flags(const float* mag, const float* sums, const CfarVArgs& cv, bool col_on,
                                              int v0, int v1, uint8_t* __restrict__ out, size_t R, bool rv) {
    out += (size_t)v0 * R;
    for (int v = v0; v < v1; ++v) {
        const uint8_t f = doppler_test(mag, sums, cv, col_on, v);
        if (rv) *out = f;
        out += R;
    }
}

// The run of Doppler rows a CFAR thread takes: runs 0 and G-1 (the only ones near the column's
// ends with the reference's full row band, whose windows need the one-sided selects) go to the
// first wave's threads, so one wave of the workgroup runs the edge path instead of two.
template <int G, int W>
__device__ __forceinline__ int cfar_run(int g) {
    if constexpr (64 % W == 0 && 64 / W >= 2 && G > 2) return g == 0 ? 0 : (g == 1 ? G - 1 : g - 1);
    else return g;
}

// Threads first, first + step, ... evaluate the hits of region rg: REF/SAVE > 0 compile-time
// windows (every load of a hit's window issues at once); 0: the runtime ref/save of CfarRArgs.
template <int REF, int SAVE>
__device__ __forceinline__ void cfar_hit_region(const float* __restrict__ rdm, uint8_t* __restrict__ flag,
                                                const uint32_t* __restrict__ hits,
                                                const uint32_t* __restrict__ counts, int rg, int region,
                                                const CfarRArgs& a, int first, int step = 64) {
    const uint32_t n = counts[rg];
    const uint32_t* list = hits + (size_t)rg * region;
    const int R = a.R, V = a.V;
    const int ref = REF > 0 ? REF : a.ref, save = REF > 0 ? SAVE : a.save;
    for (uint32_t i = first; i < n; i += step) {
        const uint32_t idx = list[i];
        const uint32_t row = idx / (uint32_t)R;        // cpi * V + v
        const int r = (int)(idx - row * (uint32_t)R);
        const int v = (int)(row % (uint32_t)V);
        int slo, shi;
        seg_of(r, a.nseg, a.seg_lo, a.seg_hi, slo, shi);
        if (shi <= slo) continue;
        const bool zrow = v >= a.cz_lo && v < a.cz_hi;
        const float* xr = rdm + (size_t)row * R;
        auto X = [&](int c) { return (!zrow && c >= 0 && c < R) ? xr[c] : 0.f; };
        int best = -1;
        float bx = 0.f;
#pragma unroll
        for (int e = -1; e <= 1; ++e) {
            const int q = r + e;
            float sl = 0.f, sr = 0.f;
            if constexpr (REF > 0) {
#pragma unroll
                for (int k = 0; k < REF; ++k) {
                    sl += X(q - SAVE - REF + k);
                    sr += X(q + SAVE + 1 + k);
                }
            } else {
                for (int k = 0; k < ref; ++k) {
                    sl += X(q - save - ref + k);
                    sr += X(q + save + 1 + k);
                }
            }
            const bool lok = q - save - ref >= slo, rok = q + save + ref < shi;
            const float xq = X(q);
            if (q >= slo && q < shi && cfar_test(xq, sl, sr, lok, rok, a.method, a.Tr) && (best < 0 || xq > bx)) {
                best = q;
                bx = xq;
            }
        }
        if (best >= 0) flag[(size_t)row * R + best] = 1;
    }
}

// Where a range job reads and writes: the previous chunk's RDM / flag planes, hit lists and
// counts (MtdArgs::prev_*).
struct RangeSrc {
    const float* rdm;
    uint8_t* flag;
    const uint32_t* hits;
    const uint32_t* count;
    int region;
    const CfarRArgs& cr;
    __device__ __forceinline__ static RangeSrc of(const MtdArgs& a) {
        return RangeSrc{a.prev_rdm, a.prev_flag, a.prev_hits, a.prev_count, a.prev_region, a.prev_cr};
    }
};

// The range-stage share of one MTD workgroup for the reference's window (5 reference + 7 guard
// cells, executeCFAR.m:45-84 with Function_CFAR1D_sub_fixCells.m:34-58): its region's first
// blockDim hits, one per thread.  The hit count and the thread's hit index are loaded before
// the tile, the 17 RDM cells of the hit's row that the test reads (r-13 .. r-7, r-1 .. r+1,
// r+7 .. r+13) right after the tile's own loads,
// and the test + first-maximum scatter run after the tile -- the three dependent gathers hide
// under the tile's FFT and Doppler CFAR instead of trailing the workgroup.
struct RangeJob57 {
    // the cells executeCFAR's fixCells test of r-1, r, r+1 reads (5 reference cells beyond 7 guard
    // cells on each side): r-13 .. r-7, r-1 .. r+1, r+7 .. r+13
    static constexpr int NX = 17;
    static constexpr int kLoads = NX;   // fetch_cells' gathers (the hook of mtd_tile)
    static __device__ __forceinline__ constexpr int cell_off(int k) { return k < 7 ? k - 13 : (k < 10 ? k - 8 : k - 3); }
    // the NX cells of hit column r in row `row` (range-checked: zero outside [0, R), on a
    // zeroed row or for a lane without a hit), issued as one batch
    static __device__ __forceinline__ void gather(float (&x)[NX], __amdgpu_buffer_rsrc_t rr, uint32_t row, int r,
                                                  bool live, int R) {
        const uint32_t rowoff = row * (uint32_t)R;
        const uint32_t rlive = live ? (uint32_t)R : 0u;   // q in [0, R) of a live lane: one unsigned compare
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            const int q = r + cell_off(k);
            x[k] = buf_ld_f(rr, (uint32_t)q < rlive ? (rowoff + (uint32_t)q) * 4u : kOob, 0u);
        }
    }
    // executeCFAR.m:45-84 at hit column r: the fixCells test of r-1, r, r+1 (one-sided windows
    // at the segment edges) and the first maximum among the passing cells, or -1
    static __device__ __forceinline__ int test(const float (&x)[NX], int r, int slo, int shi, const CfarRArgs& c) {
        int best = -1;
        float bx = 0.f;
#pragma unroll
        for (int e = -1; e <= 1; ++e) {
            const int q = r + e;   // left window q-12 .. q-8 = x[e+1 ..], centre x[8+e], right q+8 .. q+12
            float sl = 0.f, sr = 0.f;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                sl += x[e + 1 + k];
                sr += x[11 + e + k];
            }
            const bool lok = q - 12 >= slo, rok = q + 12 < shi;
            const float xq = x[8 + e];
            if (q >= slo && q < shi && cfar_test(xq, sl, sr, lok, rok, c.method, c.Tr) && (best < 0 || xq > bx)) {
                best = q;
                bx = xq;
            }
        }
        return best;
    }
    uint32_t n = 0, idx = 0;
    float x[NX];
    __device__ __forceinline__ void fetch_idx(const RangeSrc& s, int rg) {
        // both loads issue at once: a region holds W*P >= blockDim entries, so the index load
        // is in bounds (and ignored) past the count -- no count -> index round trip
        n = s.count[rg];
        idx = *(s.hits + (size_t)rg * s.region + (int)threadIdx.x);
    }
    __device__ __forceinline__ void fetch_cells(const RangeSrc& s) {
        // Every wave of every MTD workgroup issues these 17 loads, unconditionally: a lane
        // without a cell (no hit, no job) loads through the buffer range check (voffset kOob:
        // 0, no memory access).  A branch around them would leave the waits of the tile's FFT
        // (vmcnt counts in issue order) merged from two paths, so a wave with hits would wait
        // for its gathers before its first butterfly (c3: 3.8 us per 16-CPI launch).
        const CfarRArgs& c = s.cr;
        const bool mine = threadIdx.x < n;
        const uint32_t R = c.R > 0 ? (uint32_t)c.R : 1u, V = c.V > 0 ? (uint32_t)c.V : 1u;   // (no job: unset)
        const uint32_t row = idx / R;
        const int r = (int)(idx - row * R);
        const int v = (int)(row % V);
        const bool zrow = v >= c.cz_lo && v < c.cz_hi;
        gather(x, buf_rsrc(s.rdm, kOob), row, r, mine && !zrow, c.R);   // (job => the RDM is < kOob bytes)
    }
    __device__ __forceinline__ void finish(const RangeSrc& s) {
        if (threadIdx.x >= n) return;
        const CfarRArgs& c = s.cr;
        const uint32_t row = idx / (uint32_t)c.R;
        const int r = (int)(idx - row * (uint32_t)c.R);
        int slo, shi;
        seg_of(r, c.nseg, c.seg_lo, c.seg_hi, slo, shi);
        if (shi <= slo) return;
        const int best = test(x, r, slo, shi, c);
        if (best >= 0) s.flag[(size_t)row * c.R + best] = 1;
    }
};

}  // namespace rsp
