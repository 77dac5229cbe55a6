// rsp_integ.hip -- post-detection integration over the CPIs of a dwell (include/rsp.h):
// rsp_integrate_dev (amplitude planes summed, fp32) and rsp_binint_dev (flag planes counted, M of N), each
// past plane shifted row by row by its Doppler row's range walk before it is added.
//
// Three launches on the caller's stream:
//   integ_plan_kernel    one workgroup walks d_slot and d_meta once and writes, per CPI b of the batch, a row
//                        of n + 3 ints: n_eff, where x_1 .. x_{n-1} live (an in-batch CPI, a ring entry, none),
//                        the ring entry b's own plane goes to (the last n-1 CPIs of a slot only) and the
//                        slot's new count (the slot's last CPI only).
//   integ_kernel<T>      the hot path: per output cell n_eff loads, one store.  The workgroups that share an
//                        L2 (ids equal modulo 8) walk the CPIs b, b+1, .. of one tile in dispatch order: the
//                        plane that is x_0 of b is x_1 of b+1 .. x_{n-1} of b+n-1, so its n reads fall
//                        together in time and in one L2.
//   integ_ring_kernel<T> after the integrate launch has read the ring: the planes that stay are copied into
//                        their ring entries (dense [V][R]) and d_meta is written.
// Nothing is combined across threads, every cell is written once by one thread, every fp32 add is a
// separate add in the stated order: the bytes do not depend on how a thread's columns are loaded (four at
// once or one by one), on the batch split or on the run.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/rsp.h"
#include "rsp_internal.h"

namespace rsp {

namespace {

constexpr int kIT = 256;          // threads of an integrate / ring workgroup
constexpr int kIQ = 4;            // consecutive columns per thread
#ifndef RSP_INTEG_GROUP
// 4: the loads of four past planes are in flight per thread before the first of them is added
// (dev-only -D for A/B against 1, one load at a time: DESIGN.md §4j)
#define RSP_INTEG_GROUP 4
#endif
constexpr int kIG = RSP_INTEG_GROUP;
constexpr int kIPlanT = 1024;     // threads of the plan workgroup
constexpr int kXcds = 8;          // L2s that workgroup ids are dealt round
constexpr int32_t kNone = INT_MIN;

// ---- plan ------------------------------------------------------------------------------------------------
// Row b: [0] n_eff, [i] (1 <= i < n) the source of x_i: j >= 0 the CPI j of this batch, -(e + 1) the ring
// entry e (counted over all slots: s * (n-1) + entry), kNone past n_eff; [n] the ring entry (same count) that
// plane b is copied to afterwards, or -1; [n+1] the slot's count after the batch when b is the slot's last
// CPI here, else -1 ([n+2] the slot then).
__global__ __launch_bounds__(kIPlanT) void integ_plan_kernel(const int32_t* __restrict__ slot, const int32_t* __restrict__ meta,
                                                             int batch, int n, int slots, int32_t* __restrict__ plan,
                                                             int32_t* __restrict__ neff_out) {
    const int stride = n + 3;
    for (int b = threadIdx.x; b < batch; b += kIPlanT) {
        int32_t* row = plan + (int64_t)b * stride;
        const int s = slot ? slot[b] : 0;
        if (s < 0 || s >= slots) {
            row[0] = 1;
            for (int i = 1; i < n; ++i) row[i] = kNone;
            row[n] = -1;
            row[n + 1] = -1;
            row[n + 2] = 0;
            if (neff_out) neff_out[b] = 1;
            continue;
        }
        // the earlier CPIs of this slot in the batch: how many, and the nearest n-1
        int before = 0;
        if (!slot) {
            before = b;
            for (int i = 1; i < n; ++i) row[i] = i <= b ? b - i : kNone;
        } else {
            for (int i = 1; i < n; ++i) row[i] = kNone;
            for (int j = b - 1; j >= 0; --j)
                if (slot[j] == s) {
                    ++before;
                    if (before < n) row[before] = j;
                }
        }
        // the later ones, as far as it matters: fewer than n-1 means plane b stays in the ring
        int after = 0;
        if (!slot) {
            after = batch - 1 - b;
        } else {
            for (int j = b + 1; j < batch && after < n; ++j) after += slot[j] == s;
        }
        int k0 = meta[2 * s];
        if (k0 < 0) k0 = 0;   // a count is never negative; one that is reads as a reset slot
        const int64_t k = (int64_t)k0 + before;
        const int neff = (int)(k + 1 < n ? k + 1 : n);
        row[0] = neff;
        for (int i = 1; i < n; ++i) {
            if (i >= neff) {
                row[i] = kNone;
            } else if (i > before) {
                const int e = (int)((k - i) % (n - 1));   // k - i >= 0 as i < n_eff <= k + 1
                row[i] = -(s * (n - 1) + e + 1);
            }
        }
        row[n] = (n > 1 && after < n - 1) ? s * (n - 1) + (int)(k % (n - 1)) : -1;
        row[n + 1] = after == 0 ? (int32_t)(k + 1) : -1;
        row[n + 2] = s;
        if (neff_out) neff_out[b] = neff;
    }
}

// ---- integrate -------------------------------------------------------------------------------------------
template <typename T>
struct Quad {
    T x[kIQ];
};

// kIQ consecutive elements from p, whose alignment is the element's only.
template <typename T>
__device__ __forceinline__ Quad<T> load_quad(const T* p) {
    Quad<T> q;
    __builtin_memcpy(&q, p, sizeof(q));
    return q;
}
template <typename T>
__device__ __forceinline__ void store_quad(T* p, const Quad<T>& q) {
    __builtin_memcpy(p, &q, sizeof(q));
}

// The term of a past plane (row pointer src, R window columns) at column r: the cell r - shift, +0 outside.
__device__ __forceinline__ float term_at(const float* src, int64_t c, int R, int) {
    return (c >= 0 && c < R) ? src[c] : 0.0f;
}
// Binary: 1 when any of the columns c - spread .. c + spread inside the window is nonzero.
__device__ __forceinline__ int term_at(const uint8_t* src, int64_t c, int R, int spread) {
    int64_t lo = c - spread, hi = c + spread;
    if (lo < 0) lo = 0;
    if (hi > R - 1) hi = R - 1;
    int any = 0;
    for (int64_t x = lo; x <= hi; ++x) any |= src[x] != 0;
    return any;
}

template <typename T>
__global__ __launch_bounds__(kIT) void integ_kernel(const T* __restrict__ in, const T* __restrict__ hist,
                                                    const int32_t* __restrict__ shift, const int32_t* __restrict__ plan,
                                                    T* __restrict__ out, IntegArgs a, int b0, int nb, int xcd) {
    constexpr bool kSum = sizeof(T) == 4;
    // Workgroup ids go round the XCDs, each with an L2 of its own: the ids that are equal modulo xcd share
    // one, and walk the CPIs of one tile before they take the next (xcd = 1: id = tile * nb + b)
    const unsigned local = blockIdx.x / (unsigned)xcd, lane = blockIdx.x % (unsigned)xcd;
    const int b = b0 + (int)(local % (unsigned)nb);
    const int64_t tile = (int64_t)(local / (unsigned)nb) * xcd + lane;
    const int64_t item = tile * kIT + threadIdx.x;
    const int Q = (a.R + kIQ - 1) / kIQ;
    if (item >= (int64_t)a.V * Q) return;
    const int v = (int)(item / Q);
    const int c0 = (int)(item - (int64_t)v * Q) * kIQ;
    const int w = a.R - c0 < kIQ ? a.R - c0 : kIQ;   // columns of this thread
    const int32_t* row = plan + (int64_t)b * (a.n + 3);
    const int neff = row[0];

    const T* x0 = in + b * a.cs + v * a.ld + c0;
    float acc[kIQ];
    int cnt[kIQ];
    if (w == kIQ) {
        const Quad<T> q = load_quad(x0);
#pragma unroll
        for (int j = 0; j < kIQ; ++j) {
            if constexpr (kSum) acc[j] = (float)q.x[j];
            else cnt[j] = q.x[j] != 0;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kIQ; ++j) {
            const T x = j < w ? x0[j] : T(0);
            if constexpr (kSum) acc[j] = (float)x;
            else cnt[j] = x != 0;
        }
    }
    // kIG terms at a time: their loads are issued together, the additions then follow in the stated order
    for (int i0 = 1; i0 < neff; i0 += kIG) {
        float t[kIG][kIQ];
        int h[kIG][kIQ];
#pragma unroll
        for (int u = 0; u < kIG; ++u) {
            const int i = i0 + u;
            if (i >= neff) break;
            const int32_t src = row[i];
            const T* p = src >= 0 ? in + src * a.cs + v * a.ld : hist + ((int64_t)(-(src + 1)) * a.V + v) * a.R;
            const int64_t sh = shift ? (int64_t)shift[(int64_t)(i - 1) * a.V + v] : 0;
            const int64_t c = (int64_t)c0 - sh;   // source column of this thread's first cell
            if constexpr (kSum) {
                if (w == kIQ && c >= 0 && c + kIQ <= a.R) {
                    const Quad<T> q = load_quad(p + c);
#pragma unroll
                    for (int j = 0; j < kIQ; ++j) t[u][j] = q.x[j];
                } else {
#pragma unroll
                    for (int j = 0; j < kIQ; ++j) t[u][j] = j < w ? term_at(p, c + j, a.R, 0) : 0.0f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < kIQ; ++j) h[u][j] = j < w ? term_at(p, c + j, a.R, a.spread) : 0;
            }
        }
#pragma unroll
        for (int u = 0; u < kIG; ++u) {
            if (i0 + u >= neff) break;
#pragma unroll
            for (int j = 0; j < kIQ; ++j) {
                if constexpr (kSum) acc[j] = acc[j] + t[u][j];
                else cnt[j] += h[u][j];
            }
        }
    }
    T* o = out + b * a.cs + v * a.ld + c0;
    Quad<T> q;
#pragma unroll
    for (int j = 0; j < kIQ; ++j) {
        if constexpr (kSum) q.x[j] = (T)acc[j];
        else q.x[j] = (T)(cnt[j] >= a.m ? 1 : 0);
    }
    if (w == kIQ) {
        store_quad(o, q);
    } else {
#pragma unroll
        for (int j = 0; j < kIQ; ++j)
            if (j < w) o[j] = q.x[j];
    }
}

// ---- ring update -----------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kIT) void integ_ring_kernel(const T* __restrict__ in, const int32_t* __restrict__ plan,
                                                         T* __restrict__ hist, int32_t* __restrict__ meta, IntegArgs a,
                                                         int b0, int nb) {
    const int b = b0 + (int)(blockIdx.x % (unsigned)nb);
    const int64_t tile = blockIdx.x / (unsigned)nb;
    const int32_t* row = plan + (int64_t)b * (a.n + 3);
    if (tile == 0 && threadIdx.x == 0 && row[a.n + 1] >= 0) meta[2 * row[a.n + 2]] = row[a.n + 1];
    const int32_t e = row[a.n];
    if (e < 0) return;
    const int64_t item = tile * kIT + threadIdx.x;
    const int Q = (a.R + kIQ - 1) / kIQ;
    if (item >= (int64_t)a.V * Q) return;
    const int v = (int)(item / Q);
    const int c0 = (int)(item - (int64_t)v * Q) * kIQ;
    const int w = a.R - c0 < kIQ ? a.R - c0 : kIQ;
    const T* x = in + b * a.cs + v * a.ld + c0;
    T* h = hist + ((int64_t)e * a.V + v) * a.R + c0;
    if (w == kIQ) {
        store_quad(h, load_quad(x));
    } else {
        for (int j = 0; j < w; ++j) h[j] = x[j];
    }
}

// Workgroups per CPI, and the CPIs one launch takes (its grid stays below 2^31 workgroups).
inline int64_t integ_tiles(const IntegArgs& a) {
    const int64_t Q = (a.R + kIQ - 1) / kIQ;
    return (a.V * Q + kIT - 1) / kIT;
}
inline int64_t integ_span(const IntegArgs& a) {
    const int64_t nb = ((int64_t)1 << 30) / (integ_tiles(a) + kXcds);
    return nb < 1 ? 1 : nb;
}

template <typename T>
hipError_t launch_integ_t(const T* in, const T* hist, const int32_t* shift, const int32_t* slot, int32_t* meta,
                          int32_t* plan, T* out, int32_t* neff, int64_t batch, const IntegArgs& a, hipStream_t st) {
    if (batch <= 0) return hipSuccess;
    hipLaunchKernelGGL(integ_plan_kernel, dim3(1), dim3(kIPlanT), 0, st, slot, meta, (int)batch, a.n, a.slots, plan, neff);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t tiles = integ_tiles(a), span = integ_span(a);
    // dev A/B: RSP_INTEG_XCD=1 takes the plain order (DESIGN.md §4j has both)
    static const int xcd = [] { const char* v = getenv("RSP_INTEG_XCD"); return v && *v == '1' ? 1 : kXcds; }();
    for (int64_t b0 = 0; b0 < batch; b0 += span) {
        const int64_t nb = batch - b0 < span ? batch - b0 : span;
        hipLaunchKernelGGL((integ_kernel<T>), dim3((unsigned)((tiles + xcd - 1) / xcd * xcd * nb)), dim3(kIT), 0, st, in, hist,
                           shift, plan, out, a, (int)b0, (int)nb, xcd);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    for (int64_t b0 = 0; b0 < batch; b0 += span) {
        const int64_t nb = batch - b0 < span ? batch - b0 : span;
        // n == 1 keeps no planes: one workgroup per CPI, for the count alone
        hipLaunchKernelGGL((integ_ring_kernel<T>), dim3((unsigned)((a.n > 1 ? tiles : 1) * nb)), dim3(kIT), 0, st, in, plan,
                           (T*)hist, meta, a, (int)b0, (int)nb);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

size_t integ_plan_bytes(int64_t batch, int n) { return (size_t)batch * (size_t)(n + 3) * sizeof(int32_t); }

hipError_t launch_integ_sum(const float* in, float* hist, const int32_t* shift, const int32_t* slot, int32_t* meta,
                            int32_t* plan, float* out, int32_t* neff, int64_t batch, const IntegArgs& a, hipStream_t st) {
    return launch_integ_t<float>(in, hist, shift, slot, meta, plan, out, neff, batch, a, st);
}

hipError_t launch_integ_bin(const uint8_t* in, uint8_t* hist, const int32_t* shift, const int32_t* slot, int32_t* meta,
                            int32_t* plan, uint8_t* out, int32_t* neff, int64_t batch, const IntegArgs& a, hipStream_t st) {
    return launch_integ_t<uint8_t>(in, hist, shift, slot, meta, plan, out, neff, batch, a, st);
}

}  // namespace rsp
