// rsp_score.hip -- detections scored against truth for gfx950: the integer reductions behind
// fun_frame_fa, fun_drate, fun_accuracy and fun_PCF (MatlabProcess_xuzerui/CFAR_WangCai/
// main_cfar.m:163-279) over a device-resident batch of V x R flag matrices and their RDMs.
// One 8-int record per CPI (include/rsp.h, rsp_score_dev); the floating-point part of the four
// functions is a few operations per CPI and runs on the host (rsp_score_summary).
//
// Up to four launches:
//   box_kernel     one workgroup per CPI.  The +-hv x +-hr detection box and fun_PCF's +-n_cell
//                  box (at most 7 x 15 and 41 x 41 cells in the reference) are clipped to the
//                  matrix for the loads, their flags summed, the status bits set to what MATLAB
//                  would have done with the unclipped ranges, and the RDM's maximum over the PCF
//                  box taken.  Writes the whole record: the final fields 1..4, zeros for the
//                  two counters the next launches add to, and -- for a CPI whose peak has to
//                  be searched -- the maximum's bits and INT_MAX in the two peak words.
//   flags_kernel   the bandwidth pass: the sum of all V x R flag bytes.  nwg workgroups per CPI,
//                  each a band of rows; 16-byte loads when the row start, the pitch and R allow
//                  it, single bytes otherwise (R = 250, or a column window at an odd offset).
//                  One integer atomic add per workgroup into the record.
//   peak_kernel    find(local_max == MTD_data) over the whole RDM, only for the CPIs that need
//                  it (valid truth, a flag in the PCF box); the other CPIs' workgroups read one
//                  word and exit.  Count by integer atomic add, first match in find() order by
//                  integer atomic min of r*V + v.
//   finish_kernel  unpacks r*V + v into (peak_v, peak_r).
// The last two run only with an RDM.  Every cross-workgroup combination is an integer add or
// min, so a record is the same whatever the schedule; no floating-point atomics, and the
// maximum's equality test is exact.  No load leaves [0, V) x [0, R).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rsp.h"
#include "rsp_internal.h"

namespace rsp {

namespace {

constexpr int kT = 256;   // threads per workgroup (4 waves)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}
__device__ __forceinline__ int wave_min(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_down(x, o, 64));
    return x;
}
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_down(x, o, 64));
    return x;
}

// Sum of the flag bytes of rows [v0, v1] x columns [r0, r1] (inclusive, already inside the
// matrix; empty when a bound pair is reversed), one cell per thread and step.
__device__ __forceinline__ int box_sum(const uint8_t* __restrict__ fl, int64_t ld, int v0, int v1, int r0, int r1) {
    if (v1 < v0 || r1 < r0) return 0;
    const int nr = r1 - r0 + 1, n = (v1 - v0 + 1) * nr;
    int s = 0;
    for (int i = threadIdx.x; i < n; i += kT) {
        const int dv = i / nr, dr = i - dv * nr;
        s += fl[(int64_t)(v0 + dv) * ld + (r0 + dr)];
    }
    return s;
}

__global__ __launch_bounds__(kT) void box_kernel(const uint8_t* __restrict__ flag, const float* __restrict__ rdm,
                                                 const int32_t* __restrict__ truth, int32_t* __restrict__ rec,
                                                 ScoreArgs a) {
    __shared__ int s_i[2][kT / 64];
    __shared__ float s_f[kT / 64];
    const int cpi = blockIdx.x;
    int32_t* out = rec + (int64_t)cpi * 8;
    const int64_t vi = truth[cpi * 3 + 0], ri = truth[cpi * 3 + 1];
    const bool valid = truth[cpi * 3 + 2] != 0;
    if (!valid) {
        if (threadIdx.x < 8) out[threadIdx.x] = 0;
        return;
    }
    const uint8_t* fl = flag + (int64_t)cpi * a.cs;
    const int64_t V = a.V, R = a.R;
    // detection box, 0-based inclusive (64-bit: a truth index may be anything)
    const int64_t bv0 = vi - a.hv, bv1 = vi + a.hv, br0 = ri - a.hr, br1 = ri + a.hr;
    const int box_status = ((bv0 < 0 || br0 < 0) ? 1 : 0) | ((bv1 >= V || br1 >= R) ? 2 : 0);
    // clipped for the loads: lower bounds into [0, size], upper into [-1, size-1] (then narrowed)
    const int n_box = box_sum(fl, a.ld, (int)min(max(bv0, (int64_t)0), V), (int)max(min(bv1, V - 1), (int64_t)-1),
                              (int)min(max(br0, (int64_t)0), R), (int)max(min(br1, R - 1), (int64_t)-1));
    // fun_PCF's box in MATLAB's 1-based indices: the chain of :248-258 clips one side at most
    const int64_t Vi = vi + 1, Ri = ri + 1, n = a.n_cell;
    int64_t pv0 = Vi - n, pv1 = Vi + n, pr0 = Ri - n, pr1 = Ri + n;
    if (Vi - n < 1) pv0 = 1;
    else if (Vi + n > a.v_lim) pv1 = a.v_lim;
    else if (Ri - n < 1) pr0 = 1;
    else if (Ri + n > a.r_lim) pr1 = a.r_lim;
    // an empty range (hi < lo) is a valid index; a non-empty one must lie in 1..size
    const bool err = (pv1 >= pv0 && (pv0 < 1 || pv1 > V)) || (pr1 >= pr0 && (pr0 < 1 || pr1 > R));
    const bool empty = pv1 < pv0 || pr1 < pr0;
    int n_pcf = 0;
    float mx = -INFINITY;
    if (!err && !empty) {   // inside the matrix: no clipping needed
        const int v0 = (int)pv0 - 1, r0 = (int)pr0 - 1, nr = (int)(pr1 - pr0) + 1, nc = (int)(pv1 - pv0 + 1) * nr;
        const float* rd = rdm ? rdm + (int64_t)cpi * a.cs : nullptr;
        for (int i = threadIdx.x; i < nc; i += kT) {
            const int dv = i / nr, dr = i - dv * nr;
            const int64_t off = (int64_t)(v0 + dv) * a.ld + (r0 + dr);
            n_pcf += fl[off];
            if (rd) mx = fmaxf(mx, rd[off]);   // fmaxf drops a NaN, as MATLAB's max does
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w_box = wave_sum(n_box), w_pcf = wave_sum(n_pcf);
    const float w_mx = wave_max(mx);
    if (lane == 0) {
        s_i[0][wave] = w_box;
        s_i[1][wave] = w_pcf;
        s_f[wave] = w_mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int t_box = 0, t_pcf = 0;
        float t_mx = -INFINITY;
#pragma unroll
        for (int w = 0; w < kT / 64; ++w) {
            t_box += s_i[0][w];
            t_pcf += s_i[1][w];
            t_mx = fmaxf(t_mx, s_f[w]);
        }
        const bool scan = rdm != nullptr && t_pcf > 0;
        out[0] = 0;
        out[1] = t_box;
        out[2] = box_status;
        out[3] = t_pcf;
        out[4] = err ? 1 : 0;
        out[5] = 0;
        out[6] = scan ? __float_as_int(t_mx) : 0;
        out[7] = scan ? INT_MAX : 0;
    }
}

// The band of rows of workgroup blockIdx.x of gridDim.x.
__device__ __forceinline__ void band(int V, int* v_lo, int* v_hi) {
    const int rows = (V + (int)gridDim.x - 1) / (int)gridDim.x;
    *v_lo = min(V, (int)blockIdx.x * rows);
    *v_hi = min(V, *v_lo + rows);
}

// Sum of the flag bytes of the workgroup's band.  WIDE: 16 columns per load; tx_bits = log2 of
// the threads along a row (a power of two covering the row's loads, at most 256), the other
// 256 >> tx_bits thread rows step down the band.
template <bool WIDE>
__global__ __launch_bounds__(kT) void flags_kernel(const uint8_t* __restrict__ flag, int32_t* __restrict__ rec,
                                                   ScoreArgs a, int tx_bits) {
    __shared__ int s_w[kT / 64];
    const int cpi = blockIdx.y;
    const uint8_t* fl = flag + (int64_t)cpi * a.cs;
    int v_lo, v_hi;
    band(a.V, &v_lo, &v_hi);
    const int TX = 1 << tx_bits, TY = kT >> tx_bits;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_bits;
    const int nc = WIDE ? a.R >> 4 : a.R;   // loads per row
    uint32_t s = 0;
    for (int c = tx; c < nc; c += TX) {
#pragma unroll 8
        for (int v = v_lo + ty; v < v_hi; v += TY) {
            if constexpr (WIDE) {
                const u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(fl + (int64_t)v * a.ld) + c);
                // v_sad_u8 against 0: the four bytes of a word added up in one instruction
                s = __builtin_amdgcn_sad_u8(w.x, 0u, s);
                s = __builtin_amdgcn_sad_u8(w.y, 0u, s);
                s = __builtin_amdgcn_sad_u8(w.z, 0u, s);
                s = __builtin_amdgcn_sad_u8(w.w, 0u, s);
            } else {
                s += fl[(int64_t)v * a.ld + c];
            }
        }
    }
    const int w = wave_sum((int)s);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < kT / 64; ++k) t += s_w[k];
        if (t) atomicAdd(&rec[(int64_t)cpi * 8 + 0], t);
    }
}

// find(local_max == MTD_data) over the workgroup's band of a CPI that needs it: the number of
// matches and the smallest r*V + v.  WIDE: four columns per load.
template <bool WIDE>
__global__ __launch_bounds__(kT) void peak_kernel(const float* __restrict__ rdm, int32_t* __restrict__ rec, ScoreArgs a,
                                                  int tx_bits) {
    __shared__ int s_c[kT / 64], s_m[kT / 64];
    const int cpi = blockIdx.y;
    int32_t* out = rec + (int64_t)cpi * 8;
    if (out[3] <= 0) return;   // no flag in the PCF box (or no valid truth): nothing to search
    const float m = __int_as_float(out[6]);
    const float* rd = rdm + (int64_t)cpi * a.cs;
    int v_lo, v_hi;
    band(a.V, &v_lo, &v_hi);
    const int TX = 1 << tx_bits, TY = kT >> tx_bits;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_bits;
    const int nc = WIDE ? a.R >> 2 : a.R;
    int cnt = 0, first = INT_MAX;
    for (int c = tx; c < nc; c += TX) {
#pragma unroll 8
        for (int v = v_lo + ty; v < v_hi; v += TY) {
            if constexpr (WIDE) {
                const f32x4 w = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(rd + (int64_t)v * a.ld) + c);
                if (w.x == m || w.y == m || w.z == m || w.w == m) {   // rare: one cell per CPI as a rule
                    const float ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int j = 3; j >= 0; --j)
                        if (ws[j] == m) {
                            ++cnt;
                            first = min(first, (4 * c + j) * a.V + v);
                        }
                }
            } else {
                if (rd[(int64_t)v * a.ld + c] == m) {
                    ++cnt;
                    first = min(first, c * a.V + v);
                }
            }
        }
    }
    const int w_c = wave_sum(cnt), w_m = wave_min(first);
    if ((threadIdx.x & 63) == 0) {
        s_c[threadIdx.x >> 6] = w_c;
        s_m[threadIdx.x >> 6] = w_m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int t_c = 0, t_m = INT_MAX;
#pragma unroll
        for (int k = 0; k < kT / 64; ++k) {
            t_c += s_c[k];
            t_m = min(t_m, s_m[k]);
        }
        if (t_c) {
            atomicAdd(&out[5], t_c);
            atomicMin(&out[7], t_m);
        }
    }
}

__global__ __launch_bounds__(kT) void finish_kernel(int32_t* __restrict__ rec, int batch, int V) {
    const int cpi = blockIdx.x * kT + threadIdx.x;
    if (cpi >= batch) return;
    int32_t* out = rec + (int64_t)cpi * 8;
    if (out[3] <= 0) return;   // never searched: the peak words are already 0
    const int p = out[7];
    const bool found = out[5] > 0;
    out[6] = found ? p % V : 0;
    out[7] = found ? p / V : 0;
}

// log2 of the threads along a row: the power of two covering n loads, 1..256.
int row_threads_bits(int n) {
    int b = 0;
    while ((1 << b) < n && b < 8) ++b;
    return b;
}

// Workgroups per CPI: enough for about 8 per CU over the batch, each with at least min_rows
// rows (a band below ~16 KiB is all launch and reduction).
int bands_per_cpi(int V, int batch, int min_rows) {
    constexpr int kTarget = 2048;
    int nwg = (kTarget + batch - 1) / batch;
    const int max_nwg = (V + min_rows - 1) / min_rows;
    if (nwg > max_nwg) nwg = max_nwg;
    return nwg < 1 ? 1 : nwg;
}

}  // namespace

hipError_t launch_score(const uint8_t* flag, const float* rdm, const int32_t* truth, int32_t* rec, int batch,
                        const ScoreArgs& a, hipStream_t st) {
    if (batch <= 0) return hipSuccess;
    if (batch > 65535) {   // blockIdx.y carries the CPI
        for (int b0 = 0; b0 < batch; b0 += 65535) {
            const int n = batch - b0 < 65535 ? batch - b0 : 65535;
            const hipError_t e = launch_score(flag + (int64_t)b0 * a.cs, rdm ? rdm + (int64_t)b0 * a.cs : nullptr,
                                              truth + (int64_t)b0 * 3, rec + (int64_t)b0 * 8, n, a, st);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    hipLaunchKernelGGL(box_kernel, dim3(batch), dim3(kT), 0, st, flag, rdm, truth, rec, a);
    const bool wide_f = a.R % 16 == 0 && a.ld % 16 == 0 && a.cs % 16 == 0 && ((uintptr_t)flag & 15) == 0;
    {
        const int min_rows = (int)((16384 + a.R - 1) / a.R);
        const dim3 grid(bands_per_cpi(a.V, batch, min_rows), batch);
        if (wide_f)
            hipLaunchKernelGGL((flags_kernel<true>), grid, dim3(kT), 0, st, flag, rec, a, row_threads_bits(a.R / 16));
        else
            hipLaunchKernelGGL((flags_kernel<false>), grid, dim3(kT), 0, st, flag, rec, a, row_threads_bits(a.R));
    }
    if (rdm) {
        const bool wide_r = a.R % 4 == 0 && a.ld % 4 == 0 && a.cs % 4 == 0 && ((uintptr_t)rdm & 15) == 0;
        const int min_rows = (int)((4096 + a.R - 1) / a.R);
        const dim3 grid(bands_per_cpi(a.V, batch, min_rows), batch);
        if (wide_r)
            hipLaunchKernelGGL((peak_kernel<true>), grid, dim3(kT), 0, st, rdm, rec, a, row_threads_bits(a.R / 4));
        else
            hipLaunchKernelGGL((peak_kernel<false>), grid, dim3(kT), 0, st, rdm, rec, a, row_threads_bits(a.R));
        hipLaunchKernelGGL(finish_kernel, dim3((batch + kT - 1) / kT), dim3(kT), 0, st, rec, batch, a.V);
    }
    return hipGetLastError();
}

}  // namespace rsp
