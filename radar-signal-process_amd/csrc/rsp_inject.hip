// rsp_inject.hip -- simulated targets injected at a set signal-to-clutter ratio for gfx950:
// MatlabProcess_xuzerui/fun_SCR.m and fun_add_clutter.m (main.m:183-194), see include/rsp.h.
//   * general form (rsp_scr_dev): out = sqrt(g) .* simu + clutter on arbitrary arrays;
//   * point-target form (rsp_inject_dev): simu(m, n) = wf_s[n - start_s - delay_s] exp(j dphi m) is
//     formed on the fly, so the kernel is the pre-filters' stream: 8 B read + 8 B written per sample.
// Two launches per call:
//   inject_ps_kernel   one workgroup per CPI: the sums of row 1 of the target over each segment
//                      (P_s is taken from row 1 alone, before any scaling -- also what makes
//                      d_out == d_simu safe: row 1 is summed before any row is overwritten), the
//                      ratios 10^((SCR + seg_db)/10) and, for the point target, every pulse's
//                      phase: the pow and sincos are off the row kernel's critical path;
//   inject_row_kernel  one workgroup per (CPI, pulse) row: the row's clutter sums per segment in
//                      fp64 (wave shuffles, then one LDS step in a fixed order: no atomics, the
//                      output is bit-identical from run to run), threads 0..nseg-1 turn them into
//                      the gains (scr_gain, rsp_internal.h), every thread scales and adds.
// A row of up to kInjectRegVec accesses per thread (4096 samples with 16-byte accesses, 2048 with
// 8-byte ones) stays in registers between the reduction and the store, so each sample is loaded
// once; a longer row is read a second time, from L2 as the workgroup has just loaded it.
// Accesses are 16 bytes where R and the clutter pitch are even, 8 bytes otherwise (R = 1031).
// A wave's 64 accesses are consecutive columns, so which segment they lie in is decided once per
// wave on the scalar unit (wave_seg); only a wave that straddles a segment boundary tests every
// sample.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsp.h"
#include "rsp_internal.h"

namespace rsp {

namespace {

constexpr int kWaves = kBlock / 64;
constexpr int kMixed = -2;   // wave_seg: the wave's columns are not all in one segment or all in none

template <int VEC>
struct Vec;
template <>
struct Vec<1> {
    using type = float2;
};
template <>
struct Vec<2> {
    using type = float4;
};

__device__ __forceinline__ float2 lo2(float4 v) { return make_float2(v.x, v.y); }
__device__ __forceinline__ float2 hi2(float4 v) { return make_float2(v.z, v.w); }
__device__ __forceinline__ void zero(float2& v) { v = make_float2(0.f, 0.f); }
__device__ __forceinline__ void zero(float4& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }

// lane 0 receives the wave's sum, always in the same order
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// The segment that holds all the columns of this wave's access v (lane 0 has the first of 64
// consecutive accesses of VEC columns), -1 if they lie in none, kMixed otherwise.  Wave-uniform.
template <int VEC>
__device__ __forceinline__ int wave_seg(const InjectArgs& a, int v) {
    const int c0 = __builtin_amdgcn_readfirstlane(v) * VEC;
    int c1 = c0 + 64 * VEC;
    if (c1 > a.R) c1 = a.R;
    int in = -1;
    bool mixed = false;
#pragma unroll
    for (int s = 0; s < RSP_MAX_SEG; ++s) {
        if (s < a.nseg) {
            if (c0 >= a.lo[s] && c1 <= a.hi[s])
                in = s;
            else if (c0 < a.hi[s] && a.lo[s] < c1)
                mixed = true;
        }
    }
    return mixed ? kMixed : in;
}

// x^2 (RSP_SCR_AS_WRITTEN) or |x|^2 of one sample in fp64: the products of two fp32 values are exact there
__device__ __forceinline__ void power_of(int power, float2 x, double& p0, double& p1) {
    const double re = (double)x.x, im = (double)x.y;
    if (power == RSP_SCR_AS_WRITTEN) {
        p0 = re * re - im * im;
        p1 = (re + re) * im;
    } else {
        p0 = re * re + im * im;
        p1 = 0.0;
    }
}

// one sample added to the sums of the segment that holds column `col`, if any
__device__ __forceinline__ void accum(const InjectArgs& a, int col, float2 x, double (&acc)[RSP_MAX_SEG][2]) {
    double p0, p1;
    power_of(a.power, x, p0, p1);
#pragma unroll
    for (int s = 0; s < RSP_MAX_SEG; ++s) {
        const bool in = s < a.nseg && col >= a.lo[s] && col < a.hi[s];
        acc[s][0] += in ? p0 : 0.0;
        acc[s][1] += in ? p1 : 0.0;
    }
}
// (selects, not branches on sid: indexing acc by a run-time value would move it out of the registers)
__device__ __forceinline__ void add_to(int sid, double p0, double p1, double (&acc)[RSP_MAX_SEG][2]) {
#pragma unroll
    for (int s = 0; s < RSP_MAX_SEG; ++s) {
        acc[s][0] += sid == s ? p0 : 0.0;
        acc[s][1] += sid == s ? p1 : 0.0;
    }
}
// an access whose wave lies in segment sid (>= 0), in none (-1: nothing to add) or across a boundary
__device__ __forceinline__ void accum_v(const InjectArgs& a, int sid, int col, float2 x,
                                        double (&acc)[RSP_MAX_SEG][2]) {
    if (sid == kMixed) {
        accum(a, col, x, acc);
    } else if (sid >= 0) {
        double p0, p1;
        power_of(a.power, x, p0, p1);
        add_to(sid, p0, p1, acc);
    }
}
__device__ __forceinline__ void accum_v(const InjectArgs& a, int sid, int col, float4 x,
                                        double (&acc)[RSP_MAX_SEG][2]) {
    if (sid == kMixed) {
        accum(a, col, lo2(x), acc);
        accum(a, col + 1, hi2(x), acc);
    } else if (sid >= 0) {
        double p0, p1, q0, q1;
        power_of(a.power, lo2(x), p0, p1);
        power_of(a.power, hi2(x), q0, q1);
        add_to(sid, p0 + q0, p1 + q1, acc);
    }
}

// The point target's sample at column `col` of pulse 0 (the pulse's phase goes into the gain):
// the waveform of the segment that holds the column, dl[s] columns after the segment's start.
// The CPI's delays are four named registers and the gains stay in LDS: a local array indexed at
// run time would leave the registers.
struct Delays {
    int d0, d1, d2, d3;
    __device__ __forceinline__ int operator[](int s) const { return s == 0 ? d0 : s == 1 ? d1 : s == 2 ? d2 : d3; }
};
__device__ __forceinline__ Delays load_delays(const InjectArgs& a, int64_t b) {
    const int32_t* p = a.delay + b * RSP_MAX_SEG;
    return Delays{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ float2 target_at(const InjectArgs& a, const Delays& dl, int col) {
    float2 w = make_float2(0.f, 0.f);
#pragma unroll
    for (int s = 0; s < RSP_MAX_SEG; ++s) {
        if (s < a.nseg && dl[s] >= 0 && col >= a.lo[s] && col < a.hi[s]) {
            const int k = col - a.lo[s] - dl[s];
            if (k >= 0 && k < a.wf_off[s + 1] - a.wf_off[s]) w = a.wf[a.wf_off[s] + k];
        }
    }
    return w;
}
// ... of a wave whose columns all lie in segment sid >= 0, d that segment's delay
__device__ __forceinline__ float2 target_in(const InjectArgs& a, int d, int sid, int col) {
    const int off = sid == 0 ? a.wf_off[0] : sid == 1 ? a.wf_off[1] : sid == 2 ? a.wf_off[2] : a.wf_off[3];
    const int end = sid == 0 ? a.wf_off[1] : sid == 1 ? a.wf_off[2] : sid == 2 ? a.wf_off[3] : a.wf_off[4];
    const int lo = sid == 0 ? a.lo[0] : sid == 1 ? a.lo[1] : sid == 2 ? a.lo[2] : a.lo[3];
    const int k = col - lo - d;
    float2 w = make_float2(0.f, 0.f);
    if (d >= 0 && k >= 0 && k < end - off) w = a.wf[off + k];
    return w;
}

// the target's samples of access v: the general form's array, or the point target
template <int FORM>
__device__ __forceinline__ float2 load_x(const InjectArgs& a, const float2* srow, const Delays& dl,
                                         int sid, int v, float2*) {
    if constexpr (FORM == 0) return srow[v];
    if (sid == kMixed) return target_at(a, dl, v);
    if (sid >= 0) return target_in(a, dl[sid], sid, v);
    return make_float2(0.f, 0.f);
}
template <int FORM>
__device__ __forceinline__ float4 load_x(const InjectArgs& a, const float2* srow, const Delays& dl,
                                         int sid, int v, float4*) {
    if constexpr (FORM == 0) return reinterpret_cast<const float4*>(srow)[v];
    float2 p = make_float2(0.f, 0.f), q = p;
    if (sid == kMixed) {
        p = target_at(a, dl, 2 * v);
        q = target_at(a, dl, 2 * v + 1);
    } else if (sid >= 0) {
        const int d = dl[sid];
        p = target_in(a, d, sid, 2 * v);
        q = target_in(a, d, sid, 2 * v + 1);
    }
    return make_float4(p.x, p.y, q.x, q.y);
}

// g * x in fp32, not contracted; a real gain (ABS2, general form) is a real product
__device__ __forceinline__ float2 scale(float2 x, float2 g, bool cplx) {
#pragma clang fp contract(off)
    if (cplx) {
        const float pr = x.x * g.x, qr = x.y * g.y, pi = x.x * g.y, qi = x.y * g.x;
        return make_float2(pr - qr, pi + qi);
    }
    return make_float2(x.x * g.x, x.y * g.x);
}
__device__ __forceinline__ float2 plus(float2 y, float2 c) {
#pragma clang fp contract(off)
    return make_float2(y.x + c.x, y.y + c.y);
}

// out = g_s * x (+ c): x stays as it is in a column of no segment (fun_SCR leaves it alone)
__device__ __forceinline__ float2 apply(const InjectArgs& a, int col, float2 x, float2 c,
                                        const float2* g, bool cplx) {
    float2 gs = make_float2(1.f, 0.f);
    bool any = false;
#pragma unroll
    for (int s = 0; s < RSP_MAX_SEG; ++s) {
        if (s < a.nseg && col >= a.lo[s] && col < a.hi[s]) {
            gs = g[s];
            any = true;
        }
    }
    float2 y = any ? scale(x, gs, cplx) : x;
    if (a.add) y = plus(y, c);
    return y;
}
__device__ __forceinline__ float2 apply_v(const InjectArgs& a, int sid, int col, float2 x, float2 c,
                                          const float2* g, bool cplx) {
    if (sid == kMixed) return apply(a, col, x, c, g, cplx);
    float2 y = sid >= 0 ? scale(x, g[sid], cplx) : x;
    if (a.add) y = plus(y, c);
    return y;
}
__device__ __forceinline__ float4 apply_v(const InjectArgs& a, int sid, int col, float4 x, float4 c,
                                          const float2* g, bool cplx) {
    float2 p, q;
    if (sid == kMixed) {
        p = apply(a, col, lo2(x), lo2(c), g, cplx);
        q = apply(a, col + 1, hi2(x), hi2(c), g, cplx);
    } else {
        p = lo2(x);
        q = hi2(x);
        if (sid >= 0) {
            const float2 gs = g[sid];
            p = scale(p, gs, cplx);
            q = scale(q, gs, cplx);
        }
        if (a.add) {
            p = plus(p, lo2(c));
            q = plus(q, hi2(c));
        }
    }
    return make_float4(p.x, p.y, q.x, q.y);
}

// red[w][2s], red[w][2s+1] = wave w's sums of segment s
__device__ __forceinline__ void wave_sums_to_lds(const InjectArgs& a, const double (&acc)[RSP_MAX_SEG][2],
                                                 double (&red)[kWaves][2 * RSP_MAX_SEG]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < RSP_MAX_SEG; ++s) {
        if (s < a.nseg) {
            const double r0 = wave_sum(acc[s][0]);
            const double r1 = a.power == RSP_SCR_AS_WRITTEN ? wave_sum(acc[s][1]) : 0.0;
            if (lane == 0) {
                red[w][2 * s] = r0;
                red[w][2 * s + 1] = r1;
            }
        }
    }
}

// Per CPI: row 1 of the target summed per segment, the segments' ratios, the pulses' phases
// (InjectArgs::ps).
template <int FORM>
__global__ __launch_bounds__(kBlock) void inject_ps_kernel(const InjectArgs a, int64_t batch) {
    __shared__ double red[kWaves][2 * RSP_MAX_SEG];
    const int t = threadIdx.x;
    const int64_t stride = inject_ps_stride(a.P);
    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        double* ps = a.ps + b * stride;
        double acc[RSP_MAX_SEG][2] = {};
        if constexpr (FORM == 0) {
            const float2* srow = a.simu + b * a.P * (int64_t)a.R;
            for (int c = t; c < a.R; c += kBlock) accum(a, c, srow[c], acc);
        } else {
            const Delays dl = load_delays(a, b);
            for (int c = t; c < a.R; c += kBlock) accum(a, c, target_at(a, dl, c), acc);
            const double dphi = a.dphi[b];
            for (int m = t; m < a.P; m += kBlock) {
                double sn, cs;
                sincos(dphi * (double)m, &sn, &cs);
                ps[4 * RSP_MAX_SEG + 2 * m] = cs;
                ps[4 * RSP_MAX_SEG + 2 * m + 1] = sn;
            }
        }
        wave_sums_to_lds(a, acc, red);
        __syncthreads();
        if (t < a.nseg) {
            double s0 = 0.0, s1 = 0.0, db = 0.0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                s0 += red[w][2 * t];
                s1 += red[w][2 * t + 1];
            }
#pragma unroll
            for (int s = 0; s < RSP_MAX_SEG; ++s)
                if (t == s) db = a.db[s];
            ps[4 * t] = s0;
            ps[4 * t + 1] = s1;
            ps[4 * t + 2] = scr_lin(a.scr_db[b] + db);
            ps[4 * t + 3] = 0.0;
        }
        __syncthreads();
    }
}

// Point-target form: 4 workgroups per CU (at most 128 VGPRs).  A workgroup stores nothing until
// its whole row has arrived, so residency is what hides the latency.  The general form keeps two
// arrays in registers and stays at 3 (holding it to 128 VGPRs spills).
template <int FORM, int VEC, int K>
__global__ __launch_bounds__(kBlock, FORM == 1 ? 4 : 3) void inject_row_kernel(const InjectArgs a, int64_t rows) {
    using V = typename Vec<VEC>::type;
    __shared__ double red[kWaves][2 * RSP_MAX_SEG];
    __shared__ float2 gl[RSP_MAX_SEG];
    const int t = threadIdx.x;
    const int nvec = a.R / VEC;
    const bool cplx = FORM == 1 || a.power == RSP_SCR_AS_WRITTEN;
    const int64_t stride = inject_ps_stride(a.P);
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t b = row / a.P;
        const int m = (int)(row - b * a.P);
        const float2* crow = a.clutter + (b % a.c_batch) * a.c_cs + (int64_t)m * a.c_ld;
        const float2* srow = FORM == 0 ? a.simu + row * a.R : nullptr;
        float2* orow = a.out + row * a.R;
        // what the gain needs from the per-CPI scratch, and the delays, requested before the row is
        // summed so that they are not waited for after the barrier
        const double* ps = a.ps + b * stride;
        double ps_re = 0.0, ps_im = 0.0, ps_k = 0.0, ph_c = 1.0, ph_s = 0.0;
        if (t < a.nseg) {
            ps_re = ps[4 * t];
            ps_im = ps[4 * t + 1];
            ps_k = ps[4 * t + 2];
            if constexpr (FORM == 1) {
                ph_c = ps[4 * RSP_MAX_SEG + 2 * m];
                ph_s = ps[4 * RSP_MAX_SEG + 2 * m + 1];
            }
        }
        Delays dl{-1, -1, -1, -1};
        if constexpr (FORM == 1) dl = load_delays(a, b);

        double acc[RSP_MAX_SEG][2] = {};
        V c[K > 0 ? K : 1], x[K > 0 && FORM == 0 ? K : 1];
        int sid[K > 0 ? K : 1];
        if constexpr (K > 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int v = t + k * kBlock;
                sid[k] = wave_seg<VEC>(a, v);
                if (v < nvec) {
                    c[k] = reinterpret_cast<const V*>(crow)[v];
                    if constexpr (FORM == 0) x[k] = reinterpret_cast<const V*>(srow)[v];
                } else {
                    zero(c[k]);
                    if constexpr (FORM == 0) zero(x[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int v = t + k * kBlock;
                if (v < nvec) accum_v(a, sid[k], v * VEC, c[k], acc);
            }
        } else {
            for (int v = t; v < nvec; v += kBlock)
                accum_v(a, wave_seg<VEC>(a, v), v * VEC, reinterpret_cast<const V*>(crow)[v], acc);
        }

        wave_sums_to_lds(a, acc, red);
        __syncthreads();
        if (t < a.nseg) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                s0 += red[w][2 * t];
                s1 += red[w][2 * t + 1];
            }
            int n = 0;
#pragma unroll
            for (int s = 0; s < RSP_MAX_SEG; ++s)
                if (t == s) n = a.hi[s] - a.lo[s];
            double gr, gi;
            scr_gain(a.power, ps_re, ps_im, s0, s1, (double)n, ps_k, &gr, &gi);
            if constexpr (FORM == 1) {   // the pulse's phase exp(j dphi m), folded into the gain in fp64
                const double r = gr * ph_c - gi * ph_s, i = gr * ph_s + gi * ph_c;
                gr = r;
                gi = i;
            }
            gl[t] = make_float2((float)gr, (float)gi);
        }
        __syncthreads();
        const float2* g = gl;

        if constexpr (K > 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int v = t + k * kBlock;
                if (v < nvec) {
                    V xx;
                    if constexpr (FORM == 0)
                        xx = x[k];
                    else
                        xx = load_x<FORM>(a, srow, dl, sid[k], v, (V*)nullptr);
                    reinterpret_cast<V*>(orow)[v] = apply_v(a, sid[k], v * VEC, xx, c[k], g, cplx);
                }
            }
        } else {
            for (int v = t; v < nvec; v += kBlock) {
                const int sd = wave_seg<VEC>(a, v);
                const V cc = reinterpret_cast<const V*>(crow)[v];
                const V xx = load_x<FORM>(a, srow, dl, sd, v, (V*)nullptr);
                reinterpret_cast<V*>(orow)[v] = apply_v(a, sd, v * VEC, xx, cc, g, cplx);
            }
        }
    }
}

template <int FORM, int VEC>
hipError_t launch_rows(const InjectArgs& a, int64_t rows, hipStream_t st) {
    const int nvec = a.R / VEC;
    const int per_thread = (nvec + kBlock - 1) / kBlock;
    const int64_t cap = (int64_t)1 << 22;   // workgroups per launch; rows beyond it by grid stride
    const dim3 grid((unsigned)(rows < cap ? rows : cap)), block(kBlock);
    if (per_thread <= 2)
        hipLaunchKernelGGL((inject_row_kernel<FORM, VEC, 2>), grid, block, 0, st, a, rows);
    else if (per_thread <= kInjectRegVec)
        hipLaunchKernelGGL((inject_row_kernel<FORM, VEC, kInjectRegVec>), grid, block, 0, st, a, rows);
    else
        hipLaunchKernelGGL((inject_row_kernel<FORM, VEC, 0>), grid, block, 0, st, a, rows);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_inject(const InjectArgs& a, int64_t batch, bool vec16, hipStream_t st) {
    const int64_t rows = batch * a.P;
    if (rows == 0 || a.R == 0) return hipSuccess;
    const dim3 grid((unsigned)(batch < 65536 ? batch : 65536)), block(kBlock);
    if (a.simu)
        hipLaunchKernelGGL((inject_ps_kernel<0>), grid, block, 0, st, a, batch);
    else
        hipLaunchKernelGGL((inject_ps_kernel<1>), grid, block, 0, st, a, batch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.simu) return vec16 ? launch_rows<0, 2>(a, rows, st) : launch_rows<0, 1>(a, rows, st);
    return vec16 ? launch_rows<1, 2>(a, rows, st) : launch_rows<1, 1>(a, rows, st);
}

}  // namespace rsp
