// rsp_cmap.hip -- clutter-map detection in the zero-velocity band for gfx950.
//
// The chain writes zeros over the Doppler rows round zero velocity; this stage computes those
// rows' bins itself from the pulse-compressed rows and detects a cell against its own history.
//
//   cmap_band_kernel    a[b][k][r] = sum over beams of |sum_p tab[p][k] * pc[b][beam][p][r]|, a
//                       K x P by P x R complex product with a tiny K.  A thread owns VEC adjacent
//                       range columns and marches down the pulses: one 16-byte (VEC = 2) or
//                       8-byte (VEC = 1) load per pulse, KB complex accumulators per column in
//                       registers, the table entry tab[p][k] wave-uniform (the scalar path).  K
//                       up to 64 runs as passes of KB bins (blockIdx.y).  SPLIT = 4: the four waves
//                       of a workgroup own the same columns and a quarter of the pulses each; the
//                       quarters are added through LDS by wave 0 in quarter order.  Per column
//                       and bin the arithmetic is one fmaf chain in pulse order (four with the
//                       split), whatever VEC, KB, the grid or the batch: the bytes do not depend
//                       on any of them.
//   cmap_update_kernel  one thread per map cell of a slot: it walks the batch's CPIs in order,
//                       the map value in a register, and writes each CPI's flag.  Threads of slot
//                       0 also write the zero flags of the CPIs that update nothing.
//   cmap_age_kernel     one thread per slot, after the update (which reads the ages): age += the
//                       slot's CPIs in the batch, saturating.
// No atomics, no scratch beyond the cached table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsp.h"
#include "rsp_internal.h"

namespace rsp {

namespace {

template <int KB, int VEC, int SPLIT>
__global__ __launch_bounds__(64 * SPLIT) void cmap_band_kernel(const float2* __restrict__ pc,
                                                                const float2* __restrict__ tab, CmapArgs a,
                                                                float* __restrict__ band) {
    const int lane = threadIdx.x & 63;
    const int wave = SPLIT > 1 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) : 0;
    const int c0 = ((int)blockIdx.x * 64 + lane) * VEC;
    const bool live = c0 < a.R;   // VEC = 2 only with an even R: c0 + 1 < R as well
    const int cc = live ? c0 : 0;
    const int pass = blockIdx.y;
    const int64_t cpi = blockIdx.z;
    const int per = (a.P + SPLIT - 1) / SPLIT;
    const int p0 = wave * per, p1 = min(a.P, p0 + per);
    // pulses in flight per wave.  With 16 bins their table entries overrun the SGPRs and some
    // spill to VGPR lanes (never to scratch); measured 3-5 % faster than two pulses all the same
    constexpr int kUnroll = 4;
    float amp[KB][VEC];
#pragma unroll
    for (int k = 0; k < KB; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) amp[k][v] = 0.0f;
    for (int beam = 0; beam < a.beams; ++beam) {
        const float2* src = pc + cpi * a.cs + (int64_t)beam * a.P * a.ld + cc;
        float2 acc[KB][VEC];
#pragma unroll
        for (int k = 0; k < KB; ++k)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[k][v] = make_float2(0.0f, 0.0f);
#pragma unroll kUnroll
        for (int p = p0; p < p1; ++p) {
            float2 x[VEC];
            if constexpr (VEC == 2) {
                const float4 q = *reinterpret_cast<const float4*>(src + (int64_t)p * a.ld);
                x[0] = make_float2(q.x, q.y);
                x[1] = make_float2(q.z, q.w);
            } else {
                x[0] = src[(int64_t)p * a.ld];
            }
            const float2* t = tab + (size_t)p * a.kpad + pass * KB;
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const float2 w = t[k];
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    acc[k][v].x = fmaf(w.x, x[v].x, fmaf(-w.y, x[v].y, acc[k][v].x));
                    acc[k][v].y = fmaf(w.x, x[v].y, fmaf(w.y, x[v].x, acc[k][v].y));
                }
            }
        }
        if constexpr (SPLIT > 1) {
            // waves 1.. hand their sums to wave 0, which adds them in wave order; a quarter of the
            // bins at a time, which keeps wave 0's registers and the staging (12 KiB) small
            constexpr int KH = KB / 4;
            __shared__ float red[SPLIT - 1][KH * VEC * 2][64];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                if (wave > 0) {
#pragma unroll
                    for (int k = 0; k < KH; ++k)
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            red[wave - 1][(k * VEC + v) * 2 + 0][lane] = acc[h * KH + k][v].x;
                            red[wave - 1][(k * VEC + v) * 2 + 1][lane] = acc[h * KH + k][v].y;
                        }
                }
                __syncthreads();
                if (wave == 0) {
#pragma unroll
                    for (int s = 0; s < SPLIT - 1; ++s)
#pragma unroll
                        for (int k = 0; k < KH; ++k)
#pragma unroll
                            for (int v = 0; v < VEC; ++v) {
                                acc[h * KH + k][v].x += red[s][(k * VEC + v) * 2 + 0][lane];
                                acc[h * KH + k][v].y += red[s][(k * VEC + v) * 2 + 1][lane];
                            }
                }
                __syncthreads();   // the next quarter, and the next beam, write red again
            }
        }
#pragma unroll
        for (int k = 0; k < KB; ++k)
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                amp[k][v] += sqrtf(fmaf(acc[k][v].x, acc[k][v].x, acc[k][v].y * acc[k][v].y));
    }
    if (wave != 0 || !live) return;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const int kg = pass * KB + k;
        if (kg >= a.K) break;
        float* dst = band + (cpi * a.K + kg) * (int64_t)a.R + c0;
        if constexpr (VEC == 2) {
            *reinterpret_cast<float2*>(dst) = make_float2(amp[k][0], amp[k][1]);
        } else {
            dst[0] = amp[k][0];
        }
    }
}

constexpr int kUT = 256;
constexpr int kUB = 32;  // CPIs whose amplitudes the update loads together

__global__ __launch_bounds__(kUT) void cmap_update_kernel(const float* __restrict__ band,
                                                          const int32_t* __restrict__ slot, CmapArgs a, int64_t batch,
                                                          float* __restrict__ map, const int32_t* __restrict__ age,
                                                          uint8_t* __restrict__ flag) {
    const int64_t cells = (int64_t)a.K * a.R;
    const int64_t i = (int64_t)blockIdx.x * kUT + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= cells) return;
    const int warm = a.warmup > 1 ? a.warmup : 1;
    int n = age[s];
    float m = map[(int64_t)s * cells + i];   // not used while n == 0
    bool touched = false;
    // kUB CPIs at a time: their amplitudes are loaded together (the recursion is a dependent
    // chain, the loads are not), then applied in order
    for (int64_t b0 = 0; b0 < batch; b0 += kUB) {
        int sb[kUB];
        float x[kUB];
#pragma unroll
        for (int j = 0; j < kUB; ++j) {
            const int64_t b = b0 + j;
            sb[j] = b < batch ? (slot ? slot[b] : 0) : s + 1;   // past the batch: some other slot's
            if (sb[j] < 0 || sb[j] >= a.slots) sb[j] = -1;
            x[j] = sb[j] == s ? band[b * cells + i] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < kUB; ++j) {
            const int64_t b = b0 + j;
            if (sb[j] < 0) {
                if (s == 0 && b < batch) flag[b * cells + i] = 0;
                continue;
            }
            if (sb[j] != s) continue;
            // separate fp32 operations, as rsp.h states them: nothing is contracted into an fma
            const bool f = n >= warm && x[j] >= __fmul_rn(a.T, m);
            if (n == 0)
                m = x[j];
            else if (!(a.hold && f))
                m = __fadd_rn(m, __fmul_rn(a.w, __fsub_rn(x[j], m)));
            flag[b * cells + i] = f ? 1 : 0;
            if (n < 0x7fffffff) ++n;
            touched = true;
        }
    }
    if (touched) map[(int64_t)s * cells + i] = m;
}

__global__ __launch_bounds__(kUT) void cmap_age_kernel(const int32_t* __restrict__ slot, int slots, int64_t batch,
                                                       int32_t* __restrict__ age) {
    const int s = blockIdx.x * kUT + threadIdx.x;
    if (s >= slots) return;
    int64_t n = age[s];
    if (!slot)
        n += s == 0 ? batch : 0;
    else
        for (int64_t b = 0; b < batch; ++b) n += slot[b] == s;
    age[s] = (int32_t)(n < 0x7fffffff ? n : 0x7fffffff);
}

template <int KB, int VEC>
hipError_t band_split(const float2* pc, const float2* tab, const CmapArgs& a, dim3 grid, float* band, hipStream_t st) {
    if (a.split == 4)
        hipLaunchKernelGGL((cmap_band_kernel<KB, VEC, 4>), grid, dim3(256), 0, st, pc, tab, a, band);
    else
        hipLaunchKernelGGL((cmap_band_kernel<KB, VEC, 1>), grid, dim3(64), 0, st, pc, tab, a, band);
    return hipGetLastError();
}

}  // namespace

void cmap_plan(int64_t P, int64_t R, int64_t K, int64_t ld, int64_t cs, int* kb, int* passes, int* vec, int* split) {
    *kb = K <= 4 ? 4 : 16;
    *passes = (int)((K + *kb - 1) / *kb);
    *vec = (R % 2 == 0 && ld % 2 == 0 && cs % 2 == 0) ? 2 : 1;
    // by R and P alone: the pulse split changes the order of the sum, so it must not follow the batch
    *split = (R <= 1024 && P >= 256) ? 4 : 1;
}

hipError_t launch_cmap_band(const float2* pc, const float2* tab, const CmapArgs& a0, int batch, float* band,
                            hipStream_t st) {
    if (batch <= 0) return hipSuccess;
    CmapArgs a = a0;
    if (((uintptr_t)pc & 15) || ((uintptr_t)band & 7)) a.vec = 1;
    const int passes = a.kpad / a.kb;
    const dim3 grid((unsigned)((a.R + 64 * a.vec - 1) / (64 * a.vec)), (unsigned)passes, (unsigned)batch);
    if (a.kb == 4) {
        if (a.vec == 2) return band_split<4, 2>(pc, tab, a, grid, band, st);
        return band_split<4, 1>(pc, tab, a, grid, band, st);
    }
    if (a.vec == 2) return band_split<16, 2>(pc, tab, a, grid, band, st);
    return band_split<16, 1>(pc, tab, a, grid, band, st);
}

hipError_t launch_cmap_update(const float* band, const int32_t* slot, const CmapArgs& a, int64_t batch, float* map,
                              int32_t* age, uint8_t* flag, hipStream_t st) {
    if (batch <= 0) return hipSuccess;
    const int64_t cells = (int64_t)a.K * a.R;
    hipLaunchKernelGGL(cmap_update_kernel, dim3((unsigned)((cells + kUT - 1) / kUT), (unsigned)a.slots), dim3(kUT), 0, st,
                       band, slot, a, batch, map, (const int32_t*)age, flag);
    hipLaunchKernelGGL(cmap_age_kernel, dim3((unsigned)((a.slots + kUT - 1) / kUT)), dim3(kUT), 0, st, slot, a.slots,
                       batch, age);
    return hipGetLastError();
}

}  // namespace rsp
