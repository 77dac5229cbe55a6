// rsp_pc.hip -- pulse compression, the first kernel of the range-Doppler chain (gfx950).
//
//   pc_kernel      one workgroup per pulse (PRT) row: FIR segment(s) + frequency-domain
//                  matched filter segment(s), FFT -> x conj(replica spectrum) -> FFT, all in
//                  LDS.  Restates MTD/fun_lss_pulse_compression.m:17-80 with
//                  fun_pulse_compression.m:10-39 (linear correlation via a power-of-two
//                  FFT, SURVEY.md §8a-3 equivalence) and the DMX circular matched filter
//                  (CFAR_WangCai/DMX_SignalProcessing_main_xzr.m:348-352).
//   pc_mf_kernel   the same per matched-filter segment, specialised on its FFT length.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "rsp_fft.h"
#include "rsp_buf.h"
#include "rsp_diag.h"
#include "rsp_internal.h"
#include "rsp_pcplan.h"

namespace rsp {

// ================================================================== pulse compression
template <int N, typename TIn>
__device__ __forceinline__ void mf_segment(const TIn* __restrict__ x, float2* __restrict__ y,
                                           const SegDev& g, float2* lds, int t) {
    for (int i = t; i < N; i += kBlock) {
        float2 v = make_float2(0.f, 0.f);
        if (i < g.in_len) v = ld_c(x + g.in_start + i);
        lds[pidx(i)] = v;
    }
    __syncthreads();
    fft_lds<N, kBlock>(lds, t, g.tw);
    // Y = conj(X .* H): the inverse FFT as conj(FFT(conj(.))), 1/N folded into H
    for (int i = t; i < N; i += kBlock) lds[pidx(i)] = cconj(cmul(lds[pidx(i)], g.H[i]));
    __syncthreads();
    fft_lds<N, kBlock>(lds, t, g.tw);
    for (int i = t; i < g.out_len; i += kBlock) y[g.out_start + i] = cconj(lds[pidx(i)]);
    __syncthreads();  // lds is reused by the next segment
}

template <typename TIn>
__device__ __forceinline__ void fir_segment(const TIn* __restrict__ x, float2* __restrict__ y,
                                            const SegDev& g, int t) {
    // z[m] = scale * sum_k taps[k] x[m-k] (causal, zero state); out[n] = z[(n+shift) mod len]
    const int len = g.out_len;
    for (int n = t; n < len; n += kBlock) {
        int m = n + g.fir_shift;
        m %= len;
        float ar = 0.f, ai = 0.f;
#pragma unroll 8
        for (int k = 0; k < RSP_MAX_FIR_TAPS; ++k) {
            if (k < g.ntaps && k <= m) {
                const float2 v = ld_c(x + g.in_start + m - k);
                ar = fmaf(g.taps[k], v.x, ar);
                ai = fmaf(g.taps[k], v.y, ai);
            }
        }
        y[g.out_start + n] = make_float2(ar * g.scale, ai * g.scale);
    }
}

template <typename TIn>
__global__ __launch_bounds__(kBlock) void pc_kernel(const TIn* __restrict__ echo,
                                                    float2* __restrict__ out, PcArgs a) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int t = threadIdx.x;
    const size_t row = blockIdx.x;
    const TIn* x = echo + row * (size_t)a.R;
    float2* y = out + row * (size_t)a.R_out;
    for (int z = 0; z < a.nzero; ++z)
        for (int c = a.zero_lo[z] + t; c < a.zero_hi[z]; c += kBlock) y[c] = make_float2(0.f, 0.f);
#pragma unroll
    for (int s = 0; s < RSP_MAX_SEG; ++s) {
        if (s >= a.nseg) break;
        const SegDev& g = a.seg[s];
        if (g.kind == RSP_SEG_FIR) {
            fir_segment(x, y, g, t);
        } else {
            switch (g.nfft) {
                case 64: mf_segment<64>(x, y, g, lds, t); break;
                case 128: mf_segment<128>(x, y, g, lds, t); break;
                case 256: mf_segment<256>(x, y, g, lds, t); break;
                case 512: mf_segment<512>(x, y, g, lds, t); break;
                case 1024: mf_segment<1024>(x, y, g, lds, t); break;
                case 2048: mf_segment<2048>(x, y, g, lds, t); break;
                case 4096: mf_segment<4096>(x, y, g, lds, t); break;
                case 8192: mf_segment<8192>(x, y, g, lds, t); break;
                case 16384: mf_segment<16384>(x, y, g, lds, t); break;
                default: break;  // rejected on the host
            }
        }
    }
}

bool pc_nfft_supported(int n) {
    switch (n) {
        case 64: case 128: case 256: case 512: case 1024: case 2048: case 4096: case 8192:
        case 16384:
            return true;
        default:
            return false;
    }
}

size_t pc_lds_bytes(int max_nfft) { return (size_t)padded_len(max_nfft < 64 ? 64 : max_nfft) * sizeof(float2); }

hipError_t launch_pc(const void* echo, int dtype, float2* out, int64_t rows, const PcArgs& a,
                     size_t lds_bytes, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    static LaunchOnce once;
    hipError_t e = launch_once(once, nullptr, [](int, int*) {
        hipError_t r = hipFuncSetAttribute((const void*)pc_kernel<float2>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (r == hipSuccess)
            r = hipFuncSetAttribute((const void*)pc_kernel<__half2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    160 * 1024);
        return r;
    });
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)rows), block(kBlock);
    if (dtype == RSP_C64) {
        hipLaunchKernelGGL(pc_kernel<float2>, grid, block, lds_bytes, s, (const float2*)echo, out, a);
    } else if (dtype == RSP_C32F16) {
        hipLaunchKernelGGL(pc_kernel<__half2>, grid, block, lds_bytes, s, (const __half2*)echo, out, a);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}


// ================================================================== pulse compression v2
// One launch per matched-filter segment, specialised on its FFT length N: G threads per
// PRT row (E = N/G elements each, register-resident Stockham passes), RPB rows per
// 256..512-thread workgroup.  Row loads and stores are lane-contiguous (the strided
// element pattern of fft_reg), the spectrum multiply sits between the forward and the
// inverse FFT in registers, and the only LDS traffic is the inter-pass exchange.
template <int N>
struct PcCfg {
    // 16 elements per thread at every length: a 16384-point row is 1024 threads (4 waves per
    // SIMD, 124 VGPRs with the lean twiddles) -- 32 elements at 512 threads took 164..174 VGPRs
    // and left 2 waves per SIMD
    static constexpr int G = N / 16;                       // threads per row
    static constexpr int E = N / G;                             // elements per thread
    static constexpr int RPB = G >= 256 ? 1 : 256 / G;          // rows per workgroup
    static constexpr int T = G * RPB;
    static constexpr int SLOT = padded_len(N);
    static constexpr size_t lds = (size_t)RPB * SLOT * sizeof(float2);
};

// FIR segment of one row (fun_lss_pulse_compression.m:38-51): z = filter(b, 1, x_A) * scale
// (causal, zero initial state), out[n] = z[(n + shift) mod len].  The segment is staged in
// the row's LDS slot behind ntaps4-1 zeros, so z[m] = sum_k b_k s[kp + m - k] needs no
// bounds test.  A thread produces 4 consecutive z and walks the taps 4 at a time: 7 LDS
// reads and 16 packed fmas per step (taps pre-scaled and duplicated as (b, b), so a wave-
// uniform tap multiplies both I and Q in one v_pk_fma_f32).
__device__ __forceinline__ float2 pk_fma(float2 a, float2 b, float2 c) {
    return make_float2(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y));
}

// The FIR segment's staging loads of a wave-uniform row (G % 64 == 0): the first B*G staged
// samples (zeros before the segment and past in_len come from the buffer range check), issued
// with the row's matched-filter loads so the two share one memory round trip.
constexpr int kFirB = 8;
template <typename TIn, int G>
__device__ __forceinline__ void fir_stage_issue(float2 (&v)[kFirB], const TIn* __restrict__ x, const SegDev& g,
                                                bool valid, int t, int i0) {
    constexpr uint32_t ES = sizeof(TIn);
    const int kp = g.ntaps4 - 1;
    const auto xr = buf_rsrc(x + g.in_start, valid ? (uint32_t)g.in_len * ES : 0u);
#pragma unroll
    for (int q = 0; q < kFirB; ++q) {
        const int j = i0 + q * G - kp;
        v[q] = buf_ld_c((const TIn*)nullptr, xr, j >= 0 ? (uint32_t)j * ES : kOob, 0u);
    }
}

template <typename TIn, int G, bool WS = false>
__device__ __forceinline__ void fir_row(const TIn* __restrict__ x, float2* __restrict__ y,
                                        const SegDev& g, float* stage, bool valid, int t,
                                        const float* __restrict__ gain, bool st_ok = true,
                                        const float2* pre = nullptr) {
    float2* s2 = reinterpret_cast<float2*>(stage);
    const int kp = g.ntaps4 - 1;
    const int len = g.out_len;
    const int nst = kp + len + 4;
    if constexpr (G % 64 == 0) {
        // The row is wave-uniform: stage through a range-checked buffer resource, 8 loads per
        // thread issued together, so the staging costs one memory round trip instead of one
        // per element step; `pre` holds the first block's loads when the caller issued them.
        const auto gr = buf_rsrc(gain ? gain + g.in_start : nullptr, gain ? (uint32_t)g.in_len * 4u : 0u);
        constexpr int B = kFirB;
        for (int i0 = t; i0 < nst; i0 += B * G) {
            float2 v[B];
            if (pre && i0 == t) {
#pragma unroll
                for (int q = 0; q < B; ++q) v[q] = pre[q];
            } else {
                fir_stage_issue<TIn, G>(v, x, g, valid, t, i0);
            }
            if (gain) {   // fused iSTC (wave-uniform)
#pragma unroll
                for (int q = 0; q < B; ++q) {
                    const int j = i0 + q * G - kp;
                    v[q] = cscale(v[q], buf_ld_f(gr, j >= 0 ? (uint32_t)j * 4u : kOob, 0u));
                }
            }
#pragma unroll
            for (int q = 0; q < B; ++q)
                if (i0 + q * G < nst) s2[i0 + q * G] = v[q];
        }
    } else {
        for (int i = t; i < nst; i += G) {
            const int j = i - kp;
            float2 v = (valid && j >= 0 && j < g.in_len) ? ld_c(x + g.in_start + j) : make_float2(0.f, 0.f);
            if (gain && j >= 0 && j < g.in_len) v = cscale(v, gain[g.in_start + j]);
            s2[i] = v;
        }
    }
    xsync<WS>();
    RSP_STAMP(0, 10, false);
    const float2* __restrict__ taps = g.taps2_dev;
    for (int m0 = 4 * t; m0 < len; m0 += 4 * G) {
        float2 acc[4] = {};
        const float2* p = s2 + kp + m0;     // p[i] = x[m0 + i]
        float2 w[7];                         // w[q] = x[m0 + q - 3 - k]
        // w[4..6] of tap group k+4 are w[0..2] of group k: 4 LDS reads per group instead of 7
        w[4] = p[1];
        w[5] = p[2];
        w[6] = p[3];
        auto group = [&](int k) {
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q] = p[q - 3 - k];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const float2 b = taps[k + kk];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = pk_fma(w[i - kk + 3], b, acc[i]);
            }
            w[6] = w[2];
            w[5] = w[1];
            w[4] = w[0];
        };
        for (int k = 0; k < g.ntaps4; k += 4) group(k);
        RSP_STAMP(0, 11, false);
        if (valid && st_ok) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + i;
                if (m < len) {
                    int n = m - g.fir_shift;
                    if (n < 0) n += len;
                    *(y + g.out_start + n) = acc[i];
                }
            }
        }
    }
    RSP_STAMP(0, 12, false);
    xsync<WS>();
}

// (The long rows' input by LDS-DMA into the exchange slot, round 4's `-DRSP_PC_DMA` A/B, measured
// +0..1 % at c3 and -1.4 % at c5 and is not kept: DESIGN.md §7b; the source is in the history,
// commit e3a7a73.)

// One row's matched-filter segment (and optionally its FIR segment) by G threads.
// G >= 64: a row spans whole waves, so the row index is wave-uniform (readfirstlane makes
// that visible to the compiler) and the row's input/output spans are buffer resources in
// SGPRs -- the zero padding beyond in_len, the out_len cut and invalid rows (num_records 0)
// are the hardware range check, with no per-element branch.  G < 64 (N <= 512): rows share
// a wave, so the accesses stay per-lane predicated.
//
// ZIN / ZOUT (wave-uniform rows only, chosen by the host from the segment's lengths): the
// trailing ZIN of the thread's 16 input slices lie wholly past in_len for every thread of every
// row and sub-block -- known zero -- and the trailing ZOUT output slices lie wholly past out_len,
// never stored.  Their echo, gain and store instructions are not issued, and the first forward
// pass / last inverse pass drop the butterfly operations that only touch them (rsp_fft.h).
// Every stored value keeps its bit pattern, except that an exact zero may change sign (a dropped
// `a + 0` passes -0 through where the full form gives +0); |.|^2 and the CFAR cannot see that.
template <typename TIn, int N, int G, bool WS = false, int ZIN = 0, int ZOUT = 0>
__device__ __forceinline__ void pc_row(const TIn* __restrict__ echo, float2* __restrict__ out,
                                       const PcMfArgs& a, int row, int t, float2* buf, int sub = 0) {
    constexpr int E = N / G;
    constexpr bool kUniform = G % 64 == 0;
    static_assert((ZIN == 0 && ZOUT == 0) || kUniform, "pruned slices need a wave-uniform row");
    static_assert(ZIN >= 0 && ZIN < E && ZOUT >= 0 && ZOUT < E, "a row keeps at least one slice");
    constexpr int EI = E - ZIN, EO = E - ZOUT;   // slices that can hold input / are stored
    // Every global load of the row -- MF input and the whole spectrum slice -- is issued up
    // front, so one memory round trip overlaps the FIR (short rows) and the spectrum arrives
    // during the forward FFT instead of after it (N <= 4096: the 32 extra live VGPRs fit the
    // paired kernel's allocation, which its short-row path already sets; PC 41 -> 39.8 us per
    // 16 CPIs at c3, 39.7 -> 37.8 us per CPI at c5).  8192/16384-point rows keep the spectrum
    // loads after the forward FFT.
    constexpr bool kEarly = G <= 64 || N <= 4096;
    if constexpr (kUniform) {   // (a VGPR-held offset in a buffer resource means a waterfall loop per access)
        row = __builtin_amdgcn_readfirstlane(row);
        sub = __builtin_amdgcn_readfirstlane(sub);
    }
    const bool valid = row < a.rows;
    const TIn* x = echo + (size_t)diag_pc_src_row(row) * a.R;
    const bool st_ok = valid && !kDiagPcNoStore;
    float2* y = out + (size_t)row * a.R_out;
    int in_start = a.mf.in_start, in_len = a.mf.in_len;
    int out_start = a.mf.out_start, out_len = a.mf.out_len;
    if (a.nsub > 1) {   // overlap-save sub-block (wave-uniform): shifted input and output windows
        const int off = sub * a.sub_step;
        in_start += off;
        out_start += off;
        in_len = max(0, min(in_len - off, N));
        out_len = max(0, min(out_len - off, a.sub_step));
        if constexpr (kUniform) {
            in_len = __builtin_amdgcn_readfirstlane(in_len);
            out_len = __builtin_amdgcn_readfirstlane(out_len);
            in_start = __builtin_amdgcn_readfirstlane(in_start);
            out_start = __builtin_amdgcn_readfirstlane(out_start);
        }
    }
    const float2* __restrict__ tw = a.mf.tw;
    constexpr uint32_t ES = sizeof(TIn);
    const auto hr = buf_rsrc(a.mf.H, (uint32_t)N * 8u);
    float2 u[E];
    const int e0 = t;   // the thread's element offset in each block of G
    constexpr int NW = tw_regs<N, E>() > 0 ? tw_regs<N, E>() : 1;
    float2 w[NW];
    tw_preload<N, G, 1, E, 0, NW>(w, t, tw);
    if constexpr (kUniform) {
        const auto xr = buf_rsrc(x + in_start, valid ? (uint32_t)in_len * ES : 0u);
#pragma unroll
        for (int m = 0; m < EI; ++m) u[m] = buf_ld_c((const TIn*)nullptr, xr, (uint32_t)e0 * ES, (uint32_t)(G * m) * ES);
#pragma unroll
        for (int m = EI; m < E; ++m) u[m] = make_float2(0.f, 0.f);
    } else {
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int i = t + G * m;
            u[m] = (valid && i < in_len) ? ld_c(x + in_start + i) : make_float2(0.f, 0.f);
        }
    }
    auto apply_gain = [&] {
        if (a.gain) {   // fused iSTC (rsp_set_prefilter): echo column n times gain[n]
            const auto gr = buf_rsrc(a.gain + in_start, (uint32_t)in_len * 4u);
#pragma unroll
            for (int m = 0; m < EI; ++m) u[m] = cscale(u[m], buf_ld_f(gr, (uint32_t)e0 * 4u, (uint32_t)(G * m) * 4u));
        }
    };
    apply_gain();
    float2 hs[kEarly ? E : 1];
    if constexpr (kEarly) {
#pragma unroll
        for (int m = 0; m < E; ++m) hs[m] = buf_ld_f2(hr, (uint32_t)e0 * 8u, (uint32_t)(G * m) * 8u);
    }
    // the FIR segment's staging loads ride on the same memory round trip (a second, dependent
    // round trip made the short rows' FIR phase ~40 % of their lifetime: tools/diag_stamps.py)
    float2 fpre[kUniform ? kFirB : 1];
    if constexpr (kUniform) {
        if (a.do_fir) fir_stage_issue<TIn, G>(fpre, x, a.fir, valid, t, t);
    }
    RSP_STAMP(0, 1, true);
    // columns no segment covers stay 0: the first matched filter's args carry the ranges (nzero is
    // 0 in every other segment's), with or without a FIR
    auto zero_fill = [&] {
        for (int z = 0; z < a.nzero; ++z)
            for (int c = a.zero_lo[z] + t; c < a.zero_hi[z]; c += G) y[c] = make_float2(0.f, 0.f);
    };
    if (a.do_fir) {
        if (valid) zero_fill();
        fir_row<TIn, G, WS>(x, y, a.fir, reinterpret_cast<float*>(buf), valid, t, a.gain, st_ok,
                                kUniform ? fpre : nullptr);
    } else if (a.nzero > 0 && valid && sub == 0) {   // no FIR: of an overlap-save split row, sub-block 0
        zero_fill();
    }
    RSP_STAMP(0, 2, false);
    if constexpr (!kDiagPcNoFft) fft_reg_w<N, G, 1, E, 0, NW, WS, ZIN, 0>(u, buf, t, w);
    RSP_STAMP(0, 3, false);
    if constexpr (kEarly) {
#pragma unroll
        for (int m = 0; m < E; m += 2)   // conj(X.*H), 1/N in H (E is even)
            cmul2_conj(u[m], u[m], hs[m], u[m + 1], u[m + 1], hs[m + 1]);
    } else {
        constexpr int HB = 8;
#pragma unroll
        for (int m0 = 0; m0 < E; m0 += HB) {
            float2 h[HB];   // batches of spectrum loads, then the multiply
#pragma unroll
            for (int m = 0; m < HB; ++m) h[m] = buf_ld_f2(hr, (uint32_t)e0 * 8u, (uint32_t)(G * (m0 + m)) * 8u);
#pragma unroll
            for (int m = 0; m < HB; m += 2)   // conj(X.*H), 1/N in H
                cmul2_conj(u[m0 + m], u[m0 + m], h[m], u[m0 + m + 1], u[m0 + m + 1], h[m + 1]);
        }
    }
    RSP_STAMP(0, 4, false);
    if constexpr (!kDiagPcNoFft) fft_reg_w<N, G, 1, E, 0, NW, WS, 0, ZOUT>(u, buf, t, w);
    RSP_STAMP(0, 5, false);
    if constexpr (kUniform) {
        const auto yr = buf_rsrc(y + out_start, st_ok ? (uint32_t)out_len * 8u : 0u);
#pragma unroll
        for (int m = 0; m < EO; ++m) buf_st_f2(cconj(u[m]), yr, (uint32_t)e0 * 8u, (uint32_t)(G * m) * 8u);
    } else if (st_ok) {
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int i = t + G * m;
            if (i < out_len) *(y + out_start + i) = cconj(u[m]);
        }
    }
    RSP_STAMP(0, 6, false);
    RSP_STAMP(0, 7, true);
    RSP_STAMP_RT(0, 9);
}


// ROWS consecutive units of a wave-uniform matched-filter segment without a FIR, one after the
// other through the same G threads (rsp_set_pc_rows; the 4096-point rows).  The twiddles and the
// thread's spectrum slice are the same for every row of a launch: they are loaded once, ahead of
// a row loop that is not unrolled, instead of once per row (24 of a long row's 50 vector-memory
// instructions).  Inside the loop a row does exactly what pc_row does -- the same operations on
// the same operands in the same order, so every stored value keeps its bits.
//
// Every unit-derived value that reaches a buffer resource goes through readfirstlane, as in
// pc_row.  A unit past the end runs as an invalid row (num_records 0: loads return 0, stores are
// dropped) and still takes every barrier.
//
// The exchange slot is reused by the next row without a barrier of its own: fft_reg_w puts a
// barrier (xsync, "WAR") in front of every exchange write, so row k+1's first write waits for
// every wave to have arrived there, which each does only after its last exchange read of row k
// (lds_barrier waits lgkmcnt(0) before s_barrier).  (With RSP_DIAG_PC_NOFFT there is no exchange.)
template <typename TIn, int N, int G, int ROWS, int ZIN = 0, int ZOUT = 0>
__device__ __forceinline__ void pc_rows(const TIn* __restrict__ echo, float2* __restrict__ out,
                                        const PcMfArgs& a, int u0, int t, float2* buf) {
    constexpr int E = N / G;
    static_assert(G % 64 == 0 && G > 64, "rows of whole waves, exchanged through the workgroup barrier");
    static_assert(N <= 4096, "the spectrum slice stays in registers");
    static_assert(ZIN >= 0 && ZIN < E && ZOUT >= 0 && ZOUT < E, "a row keeps at least one slice");
    constexpr int EI = E - ZIN, EO = E - ZOUT;
    constexpr uint32_t ES = sizeof(TIn);
    const int e0 = t;
    const float2* __restrict__ tw = a.mf.tw;
    const auto hr = buf_rsrc(a.mf.H, (uint32_t)N * 8u);
    constexpr int NW = tw_regs<N, E>() > 0 ? tw_regs<N, E>() : 1;
    float2 w[NW];
    tw_preload<N, G, 1, E, 0, NW>(w, t, tw);
    float2 hs[E];
#pragma unroll
    for (int m = 0; m < E; ++m) hs[m] = buf_ld_f2(hr, (uint32_t)e0 * 8u, (uint32_t)(G * m) * 8u);
    const int ns = a.nsub > 1 ? a.nsub : 1;
#pragma unroll 1
    for (int k = 0; k < ROWS; ++k) {
        const int unit = __builtin_amdgcn_readfirstlane(u0 + k);
        const int row = __builtin_amdgcn_readfirstlane(unit / ns);
        const int sub = __builtin_amdgcn_readfirstlane(unit % ns);
        const bool valid = row < a.rows;
        const TIn* x = echo + (size_t)diag_pc_src_row(row) * a.R;
        const bool st_ok = valid && !kDiagPcNoStore;
        float2* y = out + (size_t)row * a.R_out;
        int in_start = a.mf.in_start, in_len = a.mf.in_len;
        int out_start = a.mf.out_start, out_len = a.mf.out_len;
        if (a.nsub > 1) {   // overlap-save sub-block: shifted input and output windows
            const int off = sub * a.sub_step;
            in_start = __builtin_amdgcn_readfirstlane(in_start + off);
            out_start = __builtin_amdgcn_readfirstlane(out_start + off);
            in_len = __builtin_amdgcn_readfirstlane(max(0, min(in_len - off, N)));
            out_len = __builtin_amdgcn_readfirstlane(max(0, min(out_len - off, a.sub_step)));
        }
        float2 u[E];
        const auto xr = buf_rsrc(x + in_start, valid ? (uint32_t)in_len * ES : 0u);
#pragma unroll
        for (int m = 0; m < EI; ++m) u[m] = buf_ld_c((const TIn*)nullptr, xr, (uint32_t)e0 * ES, (uint32_t)(G * m) * ES);
#pragma unroll
        for (int m = EI; m < E; ++m) u[m] = make_float2(0.f, 0.f);
        if (a.gain) {   // fused iSTC (rsp_set_prefilter): echo column n times gain[n]
            const auto gr = buf_rsrc(a.gain + in_start, (uint32_t)in_len * 4u);
#pragma unroll
            for (int m = 0; m < EI; ++m) u[m] = cscale(u[m], buf_ld_f(gr, (uint32_t)e0 * 4u, (uint32_t)(G * m) * 4u));
        }
        if (a.nzero > 0 && valid && sub == 0) {   // columns no segment covers stay 0 (as pc_row, no FIR)
            for (int z = 0; z < a.nzero; ++z)
                for (int c = a.zero_lo[z] + t; c < a.zero_hi[z]; c += G) y[c] = make_float2(0.f, 0.f);
        }
        if constexpr (!kDiagPcNoFft) fft_reg_w<N, G, 1, E, 0, NW, false, ZIN, 0>(u, buf, t, w);
#pragma unroll
        for (int m = 0; m < E; m += 2)   // conj(X.*H), 1/N in H (E is even)
            cmul2_conj(u[m], u[m], hs[m], u[m + 1], u[m + 1], hs[m + 1]);
        if constexpr (!kDiagPcNoFft) fft_reg_w<N, G, 1, E, 0, NW, false, 0, ZOUT>(u, buf, t, w);
        const auto yr = buf_rsrc(y + out_start, st_ok ? (uint32_t)out_len * 8u : 0u);
#pragma unroll
        for (int m = 0; m < EO; ++m) buf_st_f2(cconj(u[m]), yr, (uint32_t)e0 * 8u, (uint32_t)(G * m) * 8u);
    }
}


// Workgroup size shared by a pair of segment lengths: both run T threads (RPB = T/G rows).
template <int N1, int N2>
struct PairCfg {
    static constexpr int T0 = PcCfg<N1>::G > PcCfg<N2>::G ? PcCfg<N1>::G : PcCfg<N2>::G;
    static constexpr int T = T0 < 256 ? 256 : T0;
    static constexpr int RPB1 = T / PcCfg<N1>::G, RPB2 = T / PcCfg<N2>::G;
    static constexpr size_t L1 = (size_t)RPB1 * PcCfg<N1>::SLOT * sizeof(float2);
    static constexpr size_t L2 = (size_t)RPB2 * PcCfg<N2>::SLOT * sizeof(float2);
    static constexpr size_t lds = L1 > L2 ? L1 : L2;
};

// Single segment (N2 == 0) or two independent segments in one launch: blocks
// [0, nblk2) run segment 2 (the long one, first for a short tail), the rest segment 1.
// `bid` is the block's index among the PC blocks of the launch.
// PR packs the pruned slice counts of the two segments, one hex digit each: 0x<ZIN1><ZOUT1><ZIN2><ZOUT2>
// (pc_row); 0 is the generic instance.
// ROWS > 1 (the 4096-point rows without a FIR only): a long-row workgroup walks ROWS consecutive
// units (pc_rows); the launcher sizes the long blocks by RPB * ROWS (pc_blocks).
constexpr bool pc_rows_built(int n, int rows) { return rows == 1 || (n == 4096 && (rows == 2 || rows == 4)); }
constexpr int pc_prune_code(int zi1, int zo1, int zi2, int zo2) { return zi1 << 12 | zo1 << 8 | zi2 << 4 | zo2; }
template <typename TIn, int N1, int N2, int PR = 0, int ROWS = 1>
__device__ __forceinline__ void pc_mf_block(const TIn* __restrict__ echo, float2* __restrict__ out, const PcMfArgs& a1,
                                            const PcMfArgs& a2, int nblk2, int bid, float2* lds) {
    constexpr int M2 = N2 ? N2 : N1;
    using PC = PairCfg<N1, M2>;
    // unit u of a segment = (row u / nsub, overlap-save sub-block u % nsub)
    // (CPI-to-XCD affinity of the rows was measured in round 5 and rejected:
    //  profiles/r05/affinity/ab_record.txt; the build lives in the history, commit 0cf6ef3)
    if constexpr (N2 != 0) {
        if (bid < nblk2) {
            constexpr int G = PcCfg<N2>::G;
            const int grp = threadIdx.x / G, t = threadIdx.x % G;
            const int ns = a2.nsub > 1 ? a2.nsub : 1;
            const int u = bid * PC::RPB2 + grp;
            if constexpr (ROWS > 1) {
                static_assert(pc_rows_built(N2, ROWS), "no multi-row path for this length");
                pc_rows<TIn, N2, G, ROWS, (PR >> 4 & 15), (PR & 15)>(echo, out, a2, u * ROWS, t,
                                                                     lds + grp * PcCfg<N2>::SLOT);
            } else {
                pc_row<TIn, N2, G, G == 64, (PR >> 4 & 15), (PR & 15)>(echo, out, a2, u / ns, t,
                                                                       lds + grp * PcCfg<N2>::SLOT, u % ns);
            }
            return;
        }
    }
    constexpr int G = PcCfg<N1>::G;
    const int grp = threadIdx.x / G, t = threadIdx.x % G;
    const int b = bid - (N2 ? nblk2 : 0);
    const int u = b * PC::RPB1 + grp, ns = a1.nsub > 1 ? a1.nsub : 1;   // (no FIR when ns > 1)
    // a row of one wave (G == 64) synchronises its exchanges within the wave: the rows of a
    // workgroup run independently instead of in barrier lockstep
    if constexpr (N2 == 0 && ROWS > 1) {   // a single-segment launch of long rows
        static_assert(pc_rows_built(N1, ROWS), "no multi-row path for this length");
        pc_rows<TIn, N1, G, ROWS, (PR >> 12 & 15), (PR >> 8 & 15)>(echo, out, a1, u * ROWS, t,
                                                                   lds + grp * PcCfg<N1>::SLOT);
    } else {
        pc_row<TIn, N1, G, G == 64, (PR >> 12 & 15), (PR >> 8 & 15)>(echo, out, a1, u / ns, t,
                                                                     lds + grp * PcCfg<N1>::SLOT, u % ns);
    }
}

template <typename TIn, int N1, int N2, int PR = 0, int ROWS = 1>
__global__ __launch_bounds__((PairCfg<N1, (N2 ? N2 : N1)>::T), RSP_DIAG_PC_WAVES) void pc_mf_kernel(
    const TIn* __restrict__ echo, float2* __restrict__ out, PcMfArgs a1, PcMfArgs a2, int nblk2) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    RSP_STAMP(0, 0, false);
    RSP_STAMP_RT(0, 8);
    pc_mf_block<TIn, N1, N2, PR, ROWS>(echo, out, a1, a2, nblk2, (int)blockIdx.x, lds);
}


bool pc_mf_supported(int nfft, int fir_stage_len) {
    switch (nfft) {
        case 64: case 128: case 256: case 512: case 1024: case 2048: case 4096: case 8192:
        case 16384:
            // the FIR stages its input in the row's slot
            return fir_stage_len <= padded_len(nfft);
        default:
            return false;
    }
}

template <typename TIn, int N1, int N2, int PR = 0, int ROWS = 1>
static hipError_t launch_pc_mf_n(const TIn* echo, float2* out, const PcMfArgs& a1, const PcMfArgs* a2,
                                 hipStream_t s) {
    constexpr int M2 = N2 ? N2 : N1;
    using PC = PairCfg<N1, M2>;
    static LaunchOnce once;
    constexpr size_t lds = PC::lds + kDiagPcLdsExtra;
    hipError_t e = lds_attr(once, (const void*)pc_mf_kernel<TIn, N1, N2, PR, ROWS>, lds);
    if (e != hipSuccess) return e;
    // ROWS applies to the long rows: segment 2 of a pair, segment 1 of a single-segment launch
    const int u1 = a1.rows * (a1.nsub > 1 ? a1.nsub : 1);
    const int nblk1 = pc_blocks(u1, PC::RPB1, N2 ? 1 : ROWS);
    const int u2 = a2 ? a2->rows * (a2->nsub > 1 ? a2->nsub : 1) : 0;
    const int nblk2 = N2 ? pc_blocks(u2, PC::RPB2, ROWS) : 0;
    dim3 grid((unsigned)(nblk1 + nblk2)), block(PC::T);
    hipLaunchKernelGGL((pc_mf_kernel<TIn, N1, N2, PR, ROWS>), grid, block, lds, s, echo, out, a1, a2 ? *a2 : a1, nblk2);
    return hipGetLastError();
}

#define RSP_PAIR(n1, n2) \
    if (a1.mf.nfft == n1 && a2 && a2->mf.nfft == n2) return launch_pc_mf_n<TIn, n1, n2>(echo, out, a1, a2, s)

// The pruned instance a launch of (a1, a2) runs (0: the generic one) -- the launcher's choice, and
// what rsp_pc_plan reports.  Instances exist for the built-in presets' 1024/4096 pair
// (PcMfArgs::zin / zout are what the lengths allow; an instance that prunes no more than that is
// valid): v2 at 4096 range bins -- 723 of 1024 and 3145 of 4096 points -- and v2's overlap-save
// blocks at 8192 / 16384 range bins, full input and 3397 of 4096 outputs kept.
int pc_prune_select(const PcMfArgs& a1, const PcMfArgs* a2) {
    if (a1.mf.nfft == 1024 && a2 && a2->mf.nfft == 4096 && a1.zin >= 4 && a1.zout >= 4) {
        if (a2->zin >= 3 && a2->zout >= 3) return pc_prune_code(4, 4, 3, 3);
        if (a2->zout >= 2) return pc_prune_code(4, 4, 0, 2);
    }
    return 0;
}

// Rows per long-row workgroup slot a launch of (a1, a2) runs when `want` are asked for -- the
// launcher's choice, and what rsp_get_pc_rows reports.  The multi-row path exists for 4096-point
// rows without a FIR: the long segment of the 1024/4096 pair and a single-segment launch.
int pc_rows_select(const PcMfArgs& a1, const PcMfArgs* a2, int want) {
    if (!pc_rows_valid(want) || want == 1) return 1;
    if (a2) return a1.mf.nfft == 1024 && a2->mf.nfft == 4096 && !a2->do_fir ? want : 1;
    return a1.mf.nfft == 4096 && !a1.do_fir ? want : 1;
}

// the 4096-point long rows at 1, 2 or 4 rows per workgroup slot
template <typename TIn, int N1, int N2, int PR>
static hipError_t launch_pc_mf_r(const TIn* echo, float2* out, const PcMfArgs& a1, const PcMfArgs* a2, int rows,
                                 hipStream_t s) {
    switch (rows) {
        case 4: return launch_pc_mf_n<TIn, N1, N2, PR, 4>(echo, out, a1, a2, s);
        case 2: return launch_pc_mf_n<TIn, N1, N2, PR, 2>(echo, out, a1, a2, s);
        default: return launch_pc_mf_n<TIn, N1, N2, PR, 1>(echo, out, a1, a2, s);
    }
}

template <typename TIn>
static hipError_t launch_pc_mf_t(const TIn* echo, float2* out, const PcMfArgs& a1, const PcMfArgs* a2, int want,
                                 hipStream_t s) {
    const int rows = pc_rows_select(a1, a2, want);
    switch (pc_prune_select(a1, a2)) {
        case pc_prune_code(4, 4, 3, 3):
            return launch_pc_mf_r<TIn, 1024, 4096, pc_prune_code(4, 4, 3, 3)>(echo, out, a1, a2, rows, s);
        case pc_prune_code(4, 4, 0, 2):
            return launch_pc_mf_r<TIn, 1024, 4096, pc_prune_code(4, 4, 0, 2)>(echo, out, a1, a2, rows, s);
        default: break;   // anything else runs the generic instance
    }
    if (rows > 1) {
        if (a2) return launch_pc_mf_r<TIn, 1024, 4096, 0>(echo, out, a1, a2, rows, s);
        return launch_pc_mf_r<TIn, 4096, 0, 0>(echo, out, a1, nullptr, rows, s);
    }
    // fused pairs of the built-in presets (v2 at 1024..16384 range bins, legacy)
    RSP_PAIR(1024, 1024);
    RSP_PAIR(1024, 4096);
    RSP_PAIR(1024, 8192);
    RSP_PAIR(1024, 16384);
    RSP_PAIR(512, 1024);
    if (a2) return hipErrorNotSupported;
    switch (a1.mf.nfft) {
        case 64: return launch_pc_mf_n<TIn, 64, 0>(echo, out, a1, nullptr, s);
        case 128: return launch_pc_mf_n<TIn, 128, 0>(echo, out, a1, nullptr, s);
        case 256: return launch_pc_mf_n<TIn, 256, 0>(echo, out, a1, nullptr, s);
        case 512: return launch_pc_mf_n<TIn, 512, 0>(echo, out, a1, nullptr, s);
        case 1024: return launch_pc_mf_n<TIn, 1024, 0>(echo, out, a1, nullptr, s);
        case 2048: return launch_pc_mf_n<TIn, 2048, 0>(echo, out, a1, nullptr, s);
        case 4096: return launch_pc_mf_n<TIn, 4096, 0>(echo, out, a1, nullptr, s);
        case 8192: return launch_pc_mf_n<TIn, 8192, 0>(echo, out, a1, nullptr, s);
        case 16384: return launch_pc_mf_n<TIn, 16384, 0>(echo, out, a1, nullptr, s);
        default: return hipErrorInvalidValue;
    }
}
#undef RSP_PAIR

#ifdef RSP_DIAG_STAMPS
}  // namespace rsp
// Dev-only diagnostic export (not in include/rsp.h): copy kernel k's stamps (0 = PC, 1 = MTD)
// of the last launch, kDiagSlots per workgroup, to host.
extern "C" int rsp_diag_stamps(int k, uint64_t* host, int64_t n) {
    if (k < 0 || k > 1) return -1;
    return k == 0 ? rsp::diag_fetch(host, n) : rsp::diag_fetch_mtd(host, n);
}
namespace rsp {
#endif

bool pc_pair_supported(int n1, int n2) {
    return (n1 == 1024 && (n2 == 1024 || n2 == 4096 || n2 == 8192 || n2 == 16384)) || (n1 == 512 && n2 == 1024);
}

hipError_t launch_pc_mf(const void* echo, int dtype, float2* out, const PcMfArgs& a1, const PcMfArgs* a2,
                        int pc_rows, hipStream_t s) {
    if (a1.rows <= 0) return hipSuccess;
    if (dtype == RSP_C64) return launch_pc_mf_t((const float2*)echo, out, a1, a2, pc_rows, s);
    if (dtype == RSP_C32F16) return launch_pc_mf_t((const __half2*)echo, out, a1, a2, pc_rows, s);
    return hipErrorInvalidValue;
}

}  // namespace rsp
