// rsp_width.hip -- Doppler line width per range column for gfx950:
// CFAR_WangCai/ampConstrWidthEst.m over the columns of a [V][ld] amplitude plane that carry a hit.
//
//   width_mark_kernel  one workgroup per 64 adjacent columns of a CPI: lane = column, the four
//                      waves take every fourth row of the flag window and OR its bytes.  Every
//                      d_span entry is written here: {-1, -1} for a column without a hit, {0, 0}
//                      ("pending") for one to compute; the CPI's count is one integer atomic add
//                      per workgroup (the sum of integers does not depend on the order).
//   width_kernel       one workgroup per group of 16 adjacent columns (64 bytes of a row).  It
//                      reads the group's 16 marks and leaves at once when none is pending.  The
//                      pending columns run four at a time, one per wave:
//                        load   all 256 threads gather the (up to) four columns, 64 rows per step,
//                               into LDS as float, rotated by floor(V/2) when shift is set; lanes
//                               of columns that are not pending load nothing;
//                        solve  the not-a-knot second derivatives m[0..V) in fp64.  m[1] and
//                               m[V-2] are explicit; m[2..V-3] solve the (1, 4, 1) rows by the
//                               Thomas algorithm, whose two sweeps g[i] = (rhs[i] - g[i-1]) c[i]
//                               and m[i] = g[i] - c[i] m[i+1] are first-order linear recurrences:
//                               each lane composes the affine maps of its chunk of L consecutive
//                               rows, the 64 chunk maps are scanned across the wave with shuffles,
//                               and the lane runs its chunk again from the value that enters it.
//                               c[i] = 1 / (4 - c[i-1]) is the same for every column and reaches
//                               its fixed point 2 - sqrt(3) within 32 steps: a compile-time table;
//                        scan   one pass over the (V-1) * interp + 1 samples for M1 = max(s), then
//                               blocks of 64 intervals from the front until one holds a sample with
//                               |s| >= 10^(a/20) M1, and from the back likewise.  No fine grid
//                               in memory.  interp == 1 skips the solve: s = y.
//                      The LDS arrays are indexed in chunks of L padded to an odd pitch, so the
//                      chunked sweeps (lane stride L) and the sample scan (lane stride 1) are both
//                      free of bank conflicts.
// A column's arithmetic depends on nothing but its own V amplitudes: not on the batch, the group,
// the wave it lands on or its neighbours.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsp.h"
#include "rsp_internal.h"

namespace rsp {

namespace {

constexpr int kGroup = 16;     // columns per width_kernel workgroup
constexpr int kSlots = 4;      // columns in flight per workgroup (one per wave)
constexpr int kCTab = 32;      // c[i] is at its fixed point from here on

struct CTab {
    double c[kCTab];
};
constexpr CTab make_ctab() {
    CTab t{};
    t.c[0] = 1.0 / 4.0;
    for (int i = 1; i < kCTab; ++i) t.c[i] = 1.0 / (4.0 - t.c[i - 1]);
    return t;
}
__constant__ CTab kC = make_ctab();

__global__ __launch_bounds__(kBlock) void width_mark_kernel(const uint8_t* __restrict__ flag, int V, int R, int64_t ld,
                                                             int64_t cs, int32_t* __restrict__ span,
                                                             int32_t* __restrict__ count) {
    __shared__ uint32_t s_any[kBlock / 64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = (int)blockIdx.x * 64 + lane;
    const int64_t cpi = blockIdx.y;
    const bool live = c < R;
    uint32_t any = flag ? 0u : 1u;
    if (flag && live) {
        const uint8_t* f = flag + cpi * cs + c;
        int r = wave;
        for (; r + 28 < V; r += 32) {   // eight independent loads in flight
            uint32_t x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = f[(int64_t)(r + 4 * j) * ld];
#pragma unroll
            for (int j = 0; j < 8; ++j) any |= x[j];
        }
        for (; r < V; r += 4) any |= f[(int64_t)r * ld];
    }
    s_any[wave][lane] = any;
    __syncthreads();
    if (wave != 0) return;
    any = s_any[0][lane] | s_any[1][lane] | s_any[2][lane] | s_any[3][lane];
    const bool need = live && any != 0;
    if (live) {
        const int v = need ? 0 : -1;
        span[(cpi * R + c) * 2] = v;
        span[(cpi * R + c) * 2 + 1] = v;
    }
    const unsigned long long mask = __ballot(need);
    if (lane == 0 && mask) atomicAdd(count + cpi, (int)__popcll(mask));
}

// The slot of element i in a chunk-padded LDS array: chunks of 1 << lg elements at pitch lp (odd).
__device__ __forceinline__ int phys(int i, int lg, int lp) { return (i >> lg) * lp + (i & ((1 << lg) - 1)); }

__device__ __forceinline__ double c_at(int k) { return kC.c[k < kCTab ? k : kCTab - 1]; }

struct WidthCol {
    const float* y;   // the column's amplitudes (LDS, chunk-padded)
    double* m;        // its second derivatives (LDS, chunk-padded)
    int V, lg, lp;
    __device__ __forceinline__ double yv(int i) const { return (double)y[phys(i, lg, lp)]; }
    __device__ __forceinline__ double mv(int i) const { return m[phys(i, lg, lp)]; }
};

// rhs of row i (2 <= i <= V-3) of the (1, 4, 1) system: 6 (y[i+1] - 2 y[i] + y[i-1]), less the
// known m[1] / m[V-2] in the first / last row.
__device__ __forceinline__ double width_rhs(double ym, double yc, double yp, int i, int V, double m1, double mv2) {
#pragma clang fp contract(off)
    double r = 6.0 * ((yp - 2.0 * yc) + ym);
    if (i == 2) r -= m1;
    if (i == V - 3) r -= mv2;
    return r;
}

// One wave: m[0..V) of the column (V >= 4).  The caller synchronises before and after.
__device__ void width_solve(const WidthCol& w, int lane) {
#pragma clang fp contract(off)
    const int V = w.V, L = 1 << w.lg;
    const double m1 = (w.yv(2) - 2.0 * w.yv(1)) + w.yv(0);
    const double mv2 = (w.yv(V - 1) - 2.0 * w.yv(V - 2)) + w.yv(V - 3);
    // this lane's rows [lo, hi) of the unknowns 2..V-3
    const int lo = max(lane * L, 2), hi = min((lane + 1) * L, V - 2);
    // forward sweep: g[i] = (rhs[i] - g[i-1]) c[i-2], g[1] = 0
    double A = 1.0, B = 0.0;
    if (lo < hi) {
        double ym = w.yv(lo - 1), yc = w.yv(lo);
        for (int i = lo; i < hi; ++i) {
            const double yp = w.yv(i + 1), c = c_at(i - 2);
            A = -c * A;
            B = c * (width_rhs(ym, yc, yp, i, V, m1, mv2) - B);
            ym = yc;
            yc = yp;
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {   // inclusive scan of the chunk maps, lower lanes first
        const double Ap = __shfl_up(A, d), Bp = __shfl_up(B, d);
        if (lane >= d) {
            B = A * Bp + B;
            A = A * Ap;
        }
    }
    double g = __shfl_up(B, 1);
    if (lane == 0) g = 0.0;
    A = 1.0;
    B = 0.0;
    if (lo < hi) {
        double ym = w.yv(lo - 1), yc = w.yv(lo);
        for (int i = lo; i < hi; ++i) {
            const double yp = w.yv(i + 1);
            g = c_at(i - 2) * (width_rhs(ym, yc, yp, i, V, m1, mv2) - g);
            w.m[phys(i, w.lg, w.lp)] = g;
            ym = yc;
            yc = yp;
        }
        // backward sweep over the lane's own g: m[i] = g[i] - c[i-2] m[i+1], "m[V-2]" = 0
        for (int i = hi - 1; i >= lo; --i) {
            const double c = c_at(i - 2);
            B = w.mv(i) - c * B;
            A = -c * A;
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {   // upper lanes first
        const double Ap = __shfl_down(A, d), Bp = __shfl_down(B, d);
        if (lane + d < 64) {
            B = A * Bp + B;
            A = A * Ap;
        }
    }
    double x = __shfl_down(B, 1);
    if (lane == 63) x = 0.0;
    for (int i = hi - 1; i >= lo; --i) {
        x = w.mv(i) - c_at(i - 2) * x;
        w.m[phys(i, w.lg, w.lp)] = x;
    }
    if (lane == 0) {
        w.m[phys(1, w.lg, w.lp)] = m1;
        w.m[phys(V - 2, w.lg, w.lp)] = mv2;
    }
}

// m[0] and m[V-1] from their neighbours (after the sweeps are visible).
__device__ __forceinline__ void width_ends(const WidthCol& w, int lane) {
#pragma clang fp contract(off)
    if (lane == 0) {
        const int V = w.V;
        const double a = 2.0 * w.mv(1) - w.mv(2), b = 2.0 * w.mv(V - 2) - w.mv(V - 3);
        w.m[phys(0, w.lg, w.lp)] = a;
        w.m[phys(V - 1, w.lg, w.lp)] = b;
    }
}

// The interval [j, j+1] in the local power form y_j + u (b + u (c + u d)).
struct WidthSeg {
    double y, b, c, d;
    __device__ __forceinline__ double at(double u) const { return fma(u, fma(u, fma(u, d, c), b), y); }
};
__device__ __forceinline__ WidthSeg width_seg(const WidthCol& w, int j, bool spline) {
#pragma clang fp contract(off)
    WidthSeg s;
    s.y = w.yv(j);
    s.b = s.c = s.d = 0.0;
    if (spline) {
        const double y1 = w.yv(j + 1), m0 = w.mv(j), mn = w.mv(j + 1);
        s.b = (y1 - s.y) - (2.0 * m0 + mn) / 6.0;
        s.c = m0 / 2.0;
        s.d = (mn - m0) / 6.0;
    }
    return s;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// One wave: {first, last} of the samples with |s| >= level * max(s), or {-1, -1}.
__device__ int2 width_scan(const WidthCol& w, int interp, double level, int lane) {
    const int V = w.V, n = V - 1;   // intervals; sample i = j * interp + k, and the last knot alone
    const bool spline = interp > 1;
    const double inv = 1.0 / (double)interp;
    double best = w.yv(V - 1);
    for (int j = lane; j < n; j += 64) {
        const WidthSeg s = width_seg(w, j, spline);
        best = fmax(best, s.y);
        for (int k = 1; k < interp; ++k) best = fmax(best, s.at((double)k * inv));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) best = fmax(best, __shfl_xor(best, d));
    if (!(best > 0.0)) return make_int2(-1, -1);
    const double thr = level * best;
    const int none = 0x7fffffff;
    int first = none;
    for (int j0 = 0; j0 < n && first == none; j0 += 64) {
        const int j = j0 + lane;
        int cand = none;
        if (j < n) {
            const WidthSeg s = width_seg(w, j, spline);
            if (fabs(s.y) >= thr) cand = j * interp;
            for (int k = 1; k < interp && cand == none; ++k)
                if (fabs(s.at((double)k * inv)) >= thr) cand = j * interp + k;
        }
        first = wave_min(cand);
    }
    const bool top = fabs(w.yv(V - 1)) >= thr;
    if (first == none) first = top ? n * interp : -1;
    int last = top ? n * interp : -1;
    for (int j1 = n; j1 > 0 && last < 0; j1 -= 64) {
        const int j = j1 - 1 - lane;
        int cand = -1;
        if (j >= 0) {
            const WidthSeg s = width_seg(w, j, spline);
            for (int k = interp - 1; k >= 1 && cand < 0; --k)
                if (fabs(s.at((double)k * inv)) >= thr) cand = j * interp + k;
            if (cand < 0 && fabs(s.y) >= thr) cand = j * interp;
        }
        last = wave_max(cand);
    }
    if (first < 0 || last < 0) return make_int2(-1, -1);   // the maximum itself is a sample: not reached
    return make_int2(first, last);
}

__global__ __launch_bounds__(kBlock) void width_kernel(const float* __restrict__ amp, WidthArgs a, int32_t* span) {
    extern __shared__ double smem[];
    __shared__ int s_cols[kGroup];
    __shared__ int s_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = (int)blockIdx.x * kGroup;
    const int64_t cpi = blockIdx.y;
    int32_t* sp = span + cpi * a.R * 2;
    if (wave == 0) {
        const bool need = lane < kGroup && c0 + lane < a.R && sp[(int64_t)(c0 + lane) * 2] == 0;
        const unsigned long long mask = __ballot(need);
        if (need) s_cols[__popcll(mask & ((1ull << lane) - 1))] = c0 + lane;
        if (lane == 0) s_n = (int)__popcll(mask);
    }
    __syncthreads();
    const int ncols = s_n;
    if (ncols == 0) return;
    const int V = a.V, lg = a.lg, lp = (1 << lg) | 1;
    const int pitch = a.pitch;                     // padded elements per column
    float* y_all = reinterpret_cast<float*>(smem);                       // [kSlots][pitch]
    double* m_all = smem + (size_t)kSlots * pitch / 2;                   // [kSlots][pitch], interp > 1 only
    const int half = a.shift ? V / 2 : 0;
    const float* src = amp + cpi * a.cs;
    for (int base = 0; base < ncols; base += kSlots) {
        const int nslot = min(kSlots, ncols - base);
        {   // load: thread = (row of 64, slot)
            const int slot = tid & (kSlots - 1);
            if (slot < nslot) {
                const int col = s_cols[base + slot];
                float* y = y_all + (size_t)slot * pitch;
                constexpr int kRows = kBlock / kSlots, kDeep = 8;   // eight independent loads in flight
                for (int r0 = tid >> 2; r0 < V; r0 += kRows * kDeep) {
                    float x[kDeep];
#pragma unroll
                    for (int j = 0; j < kDeep; ++j)   // past the column: row V-1 again, not stored
                        x[j] = src[(int64_t)min(r0 + j * kRows, V - 1) * a.ld + col];
#pragma unroll
                    for (int j = 0; j < kDeep; ++j) {
                        const int r = r0 + j * kRows;
                        int i = r + half;
                        if (i >= V) i -= V;
                        if (r < V) y[phys(i, lg, lp)] = x[j];
                    }
                }
            }
        }
        __syncthreads();
        WidthCol w;
        w.y = y_all + (size_t)wave * pitch;
        w.m = m_all + (size_t)wave * pitch;
        w.V = V;
        w.lg = lg;
        w.lp = lp;
        const bool mine = wave < nslot;
        if (a.interp > 1) {
            if (mine) width_solve(w, lane);
            __syncthreads();
            if (mine) width_ends(w, lane);
            __syncthreads();
        }
        if (mine) {
            const int2 r = width_scan(w, a.interp, a.level, lane);
            if (lane == 0) {
                sp[(int64_t)s_cols[base + wave] * 2] = r.x;
                sp[(int64_t)s_cols[base + wave] * 2 + 1] = r.y;
            }
        }
        __syncthreads();   // the next four columns overwrite the arrays
    }
}

LaunchOnce g_width_once;

}  // namespace

void width_geometry(int V, int* lg, int* pitch) {
    int l = 0;
    while ((64 << l) < V) ++l;
    *lg = l;
    *pitch = (((V - 1) >> l) + 1) * ((1 << l) | 1);
}

size_t width_lds_bytes(int V, int interp) {
    int lg = 0, pitch = 0;
    width_geometry(V, &lg, &pitch);
    return (size_t)kSlots * pitch * (sizeof(float) + (interp > 1 ? sizeof(double) : 0));
}

hipError_t launch_width(const float* amp, const uint8_t* flag, int batch, const WidthArgs& a0, int32_t* span,
                        int32_t* count, hipStream_t st) {
    if (batch <= 0) return hipSuccess;
    WidthArgs a = a0;
    width_geometry(a.V, &a.lg, &a.pitch);
    // the attribute is set once per device: for the longest column the stage accepts
    hipError_t e = lds_attr(g_width_once, (const void*)width_kernel, width_lds_bytes(RSP_WIDTH_MAX_V, 2));
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(count, 0, (size_t)batch * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(width_mark_kernel, dim3((unsigned)((a.R + 63) / 64), (unsigned)batch), dim3(kBlock), 0, st, flag,
                       a.V, a.R, a.ld, a.cs, span, count);
    hipLaunchKernelGGL(width_kernel, dim3((unsigned)((a.R + kGroup - 1) / kGroup), (unsigned)batch), dim3(kBlock),
                       width_lds_bytes(a.V, a.interp), st, amp, a, span);
    return hipGetLastError();
}

}  // namespace rsp
