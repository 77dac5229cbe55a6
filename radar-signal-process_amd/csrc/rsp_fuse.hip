// rsp_fuse.hip -- the stacked beams' hits fused per cell and the elevation from the beam amplitudes
// (include/rsp.h): rsp_beam_fuse_dev and rsp_beam_elev_dev.
//
//   fuse_kernel<G>  the hot path: every cell of `beams` amplitude planes and `beams` flag planes is read
//                   once, four outputs per cell are written once.  A thread owns four consecutive columns
//                   of one row of one CPI: per beam one 16-byte amplitude load and one 4-byte flag load, then
//                   one 16-byte store and up to three 4-byte stores.  It takes its cells one by one where
//                   they run past the row end or where a flag or byte-output address is not 4-byte aligned.
//                   G is the number of beams whose loads are issued before the first compare: 1 in the
//                   shipped path (the waves resident on a CU keep the memory system busy; groups of four
//                   measured 4-10 % slower at sparse flags and 17-20 % slower at 5.7 %).
//   elev_kernel     sparse: one thread per slot of rsp_motion_measure_dev's hit lists, the arithmetic of
//                   rsp_fuse_math.h on the three amplitudes round the peak beam.
// Nothing is combined across threads, every compare is the same float32 `>` in beam order on either path:
// the bytes do not depend on how a thread's columns are loaded, on the batch split or on the run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/rsp.h"
#include "rsp_fuse_math.h"
#include "rsp_internal.h"

namespace rsp {

namespace {

constexpr int kFT = 256;   // threads of a workgroup (both kernels)
constexpr int kFQ = 4;     // consecutive columns per thread
constexpr int kFG = 4;     // the A/B's other arm: four beams' loads in flight per thread before the first compare

struct Quad4 {
    float x[kFQ];
};

// The state of one cell while its beams go by, in beam order.
struct Cell {
    float m;       // the largest amplitude of all beams
    float best;    // the largest amplitude of the flagged beams
    int k;         // that beam, 255 before the first flagged one
    int cnt;       // flagged beams
};

__device__ __forceinline__ void cell_take(Cell& c, int beam, float a, unsigned f) {
    if (beam == 0) c.m = a;
    else if (a > c.m) c.m = a;
    if (f != 0) {
        ++c.cnt;
        if (c.k == 255 || a > c.best) {
            c.best = a;
            c.k = beam;
        }
    }
}

template <int G>
__global__ __launch_bounds__(kFT) void fuse_kernel(const float* __restrict__ amp, const uint8_t* __restrict__ flag,
                                                   uint8_t* __restrict__ fflag, uint8_t* __restrict__ fbeam,
                                                   float* __restrict__ famp, uint8_t* __restrict__ fcnt, int V, int R,
                                                   int beams, int min_beams, int64_t ld, int64_t bs, int64_t cs, int b0,
                                                   unsigned tiles) {
    const int b = b0 + (int)(blockIdx.x / tiles);
    const int64_t item = (int64_t)(blockIdx.x % tiles) * kFT + threadIdx.x;
    const int Q = (R + kFQ - 1) / kFQ;
    if (item >= (int64_t)V * Q) return;
    const int v = (int)(item / Q);
    const int c0 = (int)(item - (int64_t)v * Q) * kFQ;
    const int w = R - c0 < kFQ ? R - c0 : kFQ;   // columns of this thread

    const int64_t in_off = b * cs + v * ld + c0;
    const int64_t out_off = ((int64_t)b * V + v) * R + c0;
    const float* pa = amp + in_off;
    const uint8_t* pf = flag + in_off;
    // one test for all beams and all three byte planes: the low address bits of the first beam's flags,
    // of the beam stride and of the outputs
    uintptr_t low = (uintptr_t)pf | (uintptr_t)bs | (uintptr_t)(fflag + out_off) | (uintptr_t)(fbeam + out_off);
    if (fcnt) low |= (uintptr_t)(fcnt + out_off);
    const bool vec = w == kFQ && (low & 3) == 0;

    Cell c[kFQ];
#pragma unroll
    for (int j = 0; j < kFQ; ++j) c[j] = Cell{0.0f, 0.0f, 255, 0};

    if (vec) {
        for (int k0 = 0; k0 < beams; k0 += G) {
            Quad4 q[G];
            uint32_t fw[G];
#pragma unroll
            for (int u = 0; u < G; ++u) {
                if (k0 + u >= beams) break;
                __builtin_memcpy(&q[u], pa + (k0 + u) * bs, sizeof(Quad4));                       // 4-byte aligned
                fw[u] = *reinterpret_cast<const uint32_t*>(pf + (k0 + u) * bs);                  // 4-byte aligned
            }
#pragma unroll
            for (int u = 0; u < G; ++u) {
                if (k0 + u >= beams) break;
#pragma unroll
                for (int j = 0; j < kFQ; ++j) cell_take(c[j], k0 + u, q[u].x[j], (fw[u] >> (8 * j)) & 0xffu);
            }
        }
    } else {
        for (int j = 0; j < w; ++j)
            for (int k = 0; k < beams; ++k) cell_take(c[j], k, pa[k * bs + j], pf[k * bs + j]);
    }

    uint32_t wf = 0, wb = 0, wc = 0;
    Quad4 qa;
#pragma unroll
    for (int j = 0; j < kFQ; ++j) {
        const bool hit = c[j].cnt >= min_beams;
        wf |= (uint32_t)(hit ? 1 : 0) << (8 * j);
        wb |= (uint32_t)(hit ? c[j].k : 255) << (8 * j);
        wc |= (uint32_t)c[j].cnt << (8 * j);
        qa.x[j] = c[j].m;
    }
    if (vec) {
        *reinterpret_cast<uint32_t*>(fflag + out_off) = wf;
        *reinterpret_cast<uint32_t*>(fbeam + out_off) = wb;
        if (fcnt) *reinterpret_cast<uint32_t*>(fcnt + out_off) = wc;
        if (famp) __builtin_memcpy(famp + out_off, &qa, sizeof(Quad4));
    } else {
#pragma unroll
        for (int j = 0; j < kFQ; ++j) {
            if (j < w) {
                fflag[out_off + j] = (uint8_t)(wf >> (8 * j));
                fbeam[out_off + j] = (uint8_t)(wb >> (8 * j));
                if (fcnt) fcnt[out_off + j] = (uint8_t)(wc >> (8 * j));
                if (famp) famp[out_off + j] = qa.x[j];
            }
        }
    }
}

__global__ __launch_bounds__(kFT) void elev_kernel(const float* __restrict__ amp, const uint8_t* __restrict__ flag,
                                                   const uint8_t* __restrict__ fbeam, const int32_t* __restrict__ cells,
                                                   const int32_t* __restrict__ count, int64_t max_hits,
                                                   double* __restrict__ el, int64_t el_stride, int32_t* __restrict__ hb,
                                                   FuseArgs a, unsigned per_cpi) {
    const int64_t b = blockIdx.x / per_cpi;
    const int64_t i = (int64_t)(blockIdx.x % per_cpi) * kFT + threadIdx.x;
    int64_t n = count[b * 2];
    if (n > max_hits) n = max_hits;
    if (i >= n) return;
    const int64_t slot = b * max_hits + i;
    const int row = cells[slot * 2], col = cells[slot * 2 + 1];
    const bool inside = row >= 0 && row < a.V && col >= 0 && col < a.R;
    int k = inside ? fbeam[(b * a.V + row) * a.R + col] : 255;
    if (k >= a.beams) k = 255;
    const int64_t off = inside ? b * a.cs + row * a.ld + col : 0;
    int cnt = 0;
    if (hb && inside)
        for (int q = 0; q < a.beams; ++q) cnt += flag[off + q * a.bs] != 0;
    double e = __builtin_nan("");
    bool three = false;
    if (k != 255) {
        const bool mid = a.law != 0 && k > 0 && k < a.beams - 1;
        const float a0 = amp[off + k * a.bs];
        const float am = mid ? amp[off + (k - 1) * a.bs] : 0.0f;
        const float ap = mid ? amp[off + (k + 1) * a.bs] : 0.0f;
        // the three centres by selection: the table is a kernel argument, not memory to index
        double x[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < RSP_FUSE_MAX_BEAMS; ++q) {
            if (q == k - 1) x[0] = a.beam_el[q];
            if (q == k) x[1] = a.beam_el[q];
            if (q == k + 1) x[2] = a.beam_el[q];
        }
        // fuse_elev sees the peak as beam 1 of three, or as an edge beam where it is one
        e = mid ? fuse_elev(a.law, 1, 3, x, am, a0, ap, &three) : x[1];
    }
    el[slot * el_stride] = e;
    if (hb) {
        int32_t* h = hb + slot * 4;
        h[0] = k == 255 ? -1 : k;
        h[1] = cnt;
        h[2] = three ? k - 1 : -1;
        h[3] = three ? k + 1 : -1;
    }
}

// Workgroups per CPI, and the CPIs one launch takes (its grid stays below 2^31 workgroups).
inline int64_t fuse_tiles(const FuseArgs& a) {
    const int64_t Q = (a.R + kFQ - 1) / kFQ;
    return (a.V * Q + kFT - 1) / kFT;
}

template <int G>
hipError_t launch_fuse_g(const float* amp, const uint8_t* flag, uint8_t* fflag, uint8_t* fbeam, float* famp, uint8_t* fcnt,
                         int64_t batch, const FuseArgs& a, hipStream_t st) {
    const int64_t tiles = fuse_tiles(a);
    int64_t span = ((int64_t)1 << 30) / tiles;
    if (span < 1) span = 1;
    for (int64_t b0 = 0; b0 < batch; b0 += span) {
        const int64_t nb = batch - b0 < span ? batch - b0 : span;
        hipLaunchKernelGGL((fuse_kernel<G>), dim3((unsigned)(tiles * nb)), dim3(kFT), 0, st, amp, flag, fflag, fbeam, famp,
                           fcnt, a.V, a.R, a.beams, a.min_beams, a.ld, a.bs, a.cs, (int)b0, (unsigned)tiles);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_beam_fuse(const float* amp, const uint8_t* flag, uint8_t* fflag, uint8_t* fbeam, float* famp,
                            uint8_t* fcnt, int64_t batch, const FuseArgs& a, hipStream_t st) {
    if (batch <= 0) return hipSuccess;
    // dev A/B: RSP_FUSE_GROUP=4 issues the loads of four beams before the first compare (DESIGN.md §4k has both)
    static const bool four = [] { const char* v = getenv("RSP_FUSE_GROUP"); return v && *v == '4'; }();
    return four ? launch_fuse_g<kFG>(amp, flag, fflag, fbeam, famp, fcnt, batch, a, st)
                : launch_fuse_g<1>(amp, flag, fflag, fbeam, famp, fcnt, batch, a, st);
}

int64_t beam_elev_blocks(int64_t batch, int64_t max_hits) { return batch * ((max_hits + kFT - 1) / kFT); }

hipError_t launch_beam_elev(const float* amp, const uint8_t* flag, const uint8_t* fbeam, const int32_t* cells,
                            const int32_t* count, int64_t max_hits, double* el, int64_t el_stride, int32_t* hb,
                            int64_t batch, const FuseArgs& a, hipStream_t st) {
    if (batch <= 0 || max_hits <= 0) return hipSuccess;
    const int64_t per = (max_hits + kFT - 1) / kFT;
    hipLaunchKernelGGL(elev_kernel, dim3((unsigned)(per * batch)), dim3(kFT), 0, st, amp, flag, fbeam, cells, count, max_hits,
                       el, el_stride, hb, a, (unsigned)per);
    return hipGetLastError();
}

}  // namespace rsp
