// rsp_oscfar.hip -- ordered-statistic CFAR for gfx950: executeCFAR.m with the
// k-th smallest cell of a reference window in place of its mean.
//
// The test z[y] >= fl32(T * w_(k)) holds exactly when at least k window cells satisfy
// fl32(T * z_i) <= z[y] (multiplication by a positive constant is monotone in IEEE arithmetic), so
// no kernel here sorts or selects: each stages the premultiplied copy fl32(T * z) beside z once,
// and a cell costs 2 * ref compares and adds.
//
//   os_v_kernel  the Doppler test.  A tile of W = 2^lw columns x V rows, column-major in LDS as z
//                and T*z; thread (c, g) takes rows g, g + G, g + 2G, ... of column c (G = 256 / W),
//                for the loads and for the tests alike, four cells at a time so that their LDS
//                reads are in flight together.  The column pitch is V rounded up to
//                pitch % 32 == max(1, 32 / W): a 32-lane half of a wave holds min(W, 32) columns x
//                32 / W consecutive rows, which then fall on 32 distinct banks (ds_read_b32 banks
//                modulo 32 per half).  Stores flagV and, with rFlag = 0, flag.
//   os_r_kernel  the range test and the first-maximum re-localisation as a gather (every byte
//                of the window written once, by one thread).  One workgroup per tile of 1024
//                columns of a row.  It first ORs the Doppler flags within one column of its tile:
//                without a hit in reach every cell of the tile is 0 and the workgroup leaves
//                (hits are sparse, so most do).  Otherwise it stages z, T*z and the flagV bytes of
//                the tile and a halo of save + ref + 2 columns, evaluates the range test at the
//                cells next to a hit only, and resolves cell c as flagged iff some hit rr in
//                {c-1, c, c+1} of c's segment takes c as the first maximum of its passing cells.
// A flag depends on nothing but its own line's amplitudes: not on the batch or the tiling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsp_cfar_dev.h"
#include "rsp_internal.h"

namespace rsp {

namespace {

// cl, cr: the window cells on each side with T*z <= x (a missing side has taken the other's count).
__device__ __forceinline__ bool os_decide(int cl, int cr, int k, int form) {
    if (form == kOsUnion) return cl + cr >= k;
    return (form == kOsGo ? min(cl, cr) : max(cl, cr)) >= k;
}

// The test at N cells y[u] of a line whose valid part is [lo, hi): cell i of the line is z[i + off],
// and tz = T*z with the same indexing.  A side that leaves the valid part counts the other side's
// window instead, which is "the missing side takes the other's count" without a branch (validation
// keeps both from leaving at once); a cell that is not `on` computes on cell lo and reports false.
// The N cells' 2 * ref loads per step are independent, so N > 1 keeps that many LDS reads in flight.
template <int N>
__device__ __forceinline__ void os_test(const float* z, const float* tz, const int (&y)[N], const bool (&on)[N],
                                        int lo, int hi, const OsTest& t, int off, bool (&res)[N]) {
    int li[N], ri[N], cl[N], cr[N];
    float x[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const int yy = on[u] ? y[u] : lo;
        const int l1 = yy - t.save - t.ref, r1 = yy + t.save + 1;
        const bool lok = l1 >= lo, rok = r1 + t.ref <= hi;
        li[u] = (lok ? l1 : r1) + off;
        ri[u] = (rok ? r1 : l1) + off;
        x[u] = z[yy + off];
        cl[u] = cr[u] = 0;
    }
    for (int i = 0; i < t.ref; ++i) {
#pragma unroll
        for (int u = 0; u < N; ++u) {
            cl[u] += tz[li[u] + i] <= x[u] ? 1 : 0;
            cr[u] += tz[ri[u] + i] <= x[u] ? 1 : 0;
        }
    }
#pragma unroll
    for (int u = 0; u < N; ++u) res[u] = on[u] && os_decide(cl[u], cr[u], t.k, t.form);
}

constexpr int kOsCells = 4;   // cells a Doppler thread tests at a time

__global__ __launch_bounds__(kBlock) void os_v_kernel(const float* __restrict__ rdm, uint8_t* __restrict__ flag,
                                                      uint8_t* __restrict__ flagV, OsArgs a, int lw, int pitch) {
    extern __shared__ __attribute__((aligned(16))) float os_lds[];
    const int W = 1 << lw, G = kBlock >> lw;
    const int c = threadIdx.x & (W - 1), g = threadIdx.x >> lw;
    const int64_t cpi = blockIdx.y;
    const int r = (int)blockIdx.x * W + c;
    const bool rv = r < a.R;
    const int V = a.V;
    float* z = os_lds + (size_t)c * pitch;
    float* tz = os_lds + (size_t)(W + c) * pitch;
    const float* src = rdm + cpi * a.cs + (rv ? r : 0);
    const float T = a.v.T;
#pragma unroll 4
    for (int v = g; v < V; v += G) {
        const float x = (rv && !(v >= a.cz_lo && v < a.cz_hi)) ? src[(int64_t)v * a.ld] : 0.f;
        z[v] = x;
        tz[v] = __fmul_rn(T, x);
    }
    __syncthreads();
    if (!rv) return;
    const bool col_on = in_segs(r, a.nseg, a.seg_lo, a.seg_hi);
    uint8_t* fo = flag ? flag + cpi * a.cs + r : nullptr;
    uint8_t* vo = flagV ? flagV + cpi * a.fv_cs + r : nullptr;
    for (int v0 = g; v0 < V; v0 += kOsCells * G) {
        int y[kOsCells];
        bool on[kOsCells], f[kOsCells];
#pragma unroll
        for (int u = 0; u < kOsCells; ++u) {
            y[u] = v0 + u * G;
            on[u] = col_on && y[u] >= a.lo && y[u] < a.hi;
        }
        os_test<kOsCells>(z, tz, y, on, a.lo, a.hi, a.v, 0, f);
#pragma unroll
        for (int u = 0; u < kOsCells; ++u) {
            if (y[u] >= V) break;
            if (vo) vo[(int64_t)y[u] * a.fv_ld] = f[u] ? 1 : 0;
            if (fo) fo[(int64_t)y[u] * a.ld] = f[u] ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(kBlock) void os_r_kernel(const float* __restrict__ rdm, const uint8_t* __restrict__ flagV,
                                                      uint8_t* __restrict__ flag, OsArgs a, int tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char os_smem[];
    const int t = threadIdx.x;
    const int v = (int)blockIdx.x / tiles;
    const int c0 = ((int)blockIdx.x % tiles) * kOsRTile;
    const int64_t cpi = blockIdx.y;
    const int R = a.R;
    const int n = R - c0 < kOsRTile ? R - c0 : kOsRTile;   // the tile's columns [c0, c0 + n)
    uint8_t* out = flag + cpi * a.cs + (int64_t)v * a.ld;
    const uint8_t* fvg = flagV + cpi * a.fv_cs + (int64_t)v * a.fv_ld;
    int any = 0;
    if (v >= a.lo && v < a.hi)
        for (int i = t; i < n + 2; i += kBlock) {   // a hit at c-1, c or c+1 can flag c
            const int c = c0 - 1 + i;
            if (c >= 0 && c < R) any |= fvg[c];
        }
    if (!__syncthreads_or(any)) {
        for (int i = t; i < n; i += kBlock) out[c0 + i] = 0;
        return;
    }
    const int H = a.r.save + a.r.ref + 2;
    const int L = kOsRTile + 2 * H;
    // column c of the row, c0 - H <= c < c0 + n + H, is entry c + off of each of the four arrays
    const int off = H - c0;
    float* xs = reinterpret_cast<float*>(os_smem);
    float* ts = xs + L;
    uint8_t* fv = os_smem + (size_t)2 * L * sizeof(float);
    uint8_t* pass = fv + L;
    const bool zrow = v >= a.cz_lo && v < a.cz_hi;
    const float* xr = rdm + cpi * a.cs + (int64_t)v * a.ld;
    const float T = a.r.T;
    for (int i = t; i < n + 2 * H; i += kBlock) {
        const int c = c0 - H + i;
        const bool in = c >= 0 && c < R;
        const float x = (in && !zrow) ? xr[c] : 0.f;
        xs[i] = x;
        ts[i] = __fmul_rn(T, x);
        fv[i] = in ? fvg[c] : 0;
        pass[i] = 0;
    }
    __syncthreads();
    for (int i = t; i < n + 4; i += kBlock) {   // the candidates of the hits in reach: c0-2 .. c0+n+1
        const int q = c0 - 2 + i;
        if (q < 0 || q >= R || !(fv[q + off - 1] | fv[q + off] | fv[q + off + 1])) continue;
        int slo, shi;
        seg_of(q, a.nseg, a.seg_lo, a.seg_hi, slo, shi);
        if (shi <= slo) continue;
        const int y[1] = {q};
        const bool on[1] = {true};
        bool f[1];
        os_test<1>(xs, ts, y, on, slo, shi, a.r, off, f);
        pass[q + off] = f[0] ? 1 : 0;
    }
    __syncthreads();
    for (int i = t; i < n; i += kBlock) {
        const int c = c0 + i;
        int slo, shi;
        seg_of(c, a.nseg, a.seg_lo, a.seg_hi, slo, shi);
        bool f = false;
#pragma unroll
        for (int d = -1; d <= 1; ++d) {
            const int rr = c + d;   // a Doppler hit at rr tests rr-1 .. rr+1 inside its segment
            if (rr < slo || rr >= shi || !fv[rr + off]) continue;
            int best = -100;
            float bx = 0.f;
#pragma unroll
            for (int e = -1; e <= 1; ++e) {
                const int q = rr + e;
                if (q < slo || q >= shi || !pass[q + off]) continue;
                if (best == -100 || xs[q + off] > bx) {   // the first maximum
                    best = d + e;
                    bx = xs[q + off];
                }
            }
            f |= best == 0;
        }
        out[c] = f ? 1 : 0;
    }
}

LaunchOnce g_os_v_once;

}  // namespace

void os_v_geometry(int V, int* lw, int* pitch) {
    // the widest tile of 64, 32, ... columns whose z and T*z columns fit 80 KB: two workgroups per CU
    for (int l = 6; l >= 0; --l) {
        const int m = (32 >> l) > 1 ? (32 >> l) : 1;
        int p = V;
        while (p % 32 != m % 32) ++p;
        *lw = l;
        *pitch = p;
        if ((size_t)2 * (1 << l) * p * sizeof(float) <= 80 * 1024) return;
    }
}

size_t os_v_lds_bytes(int V) {
    int lw = 0, pitch = 0;
    os_v_geometry(V, &lw, &pitch);
    return (size_t)2 * (1 << lw) * pitch * sizeof(float);
}

size_t os_r_lds_bytes(const OsTest& r) {
    return (size_t)(kOsRTile + 2 * (r.save + r.ref + 2)) * (2 * sizeof(float) + 2);
}

hipError_t launch_os_v(const float* rdm, uint8_t* flag, uint8_t* flagV, int batch, const OsArgs& a, hipStream_t st) {
    if (batch <= 0) return hipSuccess;
    int lw = 0, pitch = 0;
    os_v_geometry(a.V, &lw, &pitch);
    hipError_t e = lds_attr(g_os_v_once, (const void*)os_v_kernel, 80 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(os_v_kernel, dim3((unsigned)((a.R + (1 << lw) - 1) >> lw), (unsigned)batch), dim3(kBlock),
                       os_v_lds_bytes(a.V), st, rdm, flag, flagV, a, lw, pitch);
    return hipGetLastError();
}

hipError_t launch_os_r(const float* rdm, const uint8_t* flagV, uint8_t* flag, int batch, const OsArgs& a,
                       hipStream_t st) {
    if (batch <= 0) return hipSuccess;
    const int tiles = (a.R + kOsRTile - 1) / kOsRTile;
    hipLaunchKernelGGL(os_r_kernel, dim3((unsigned)(tiles * a.V), (unsigned)batch), dim3(kBlock), os_r_lds_bytes(a.r),
                       st, rdm, flagV, flag, a, tiles);
    return hipGetLastError();
}

}  // namespace rsp
