// rsp_cfar.hip -- the CFAR kernels outside the MTD tile (gfx950).
//
//   cfar_r_kernel  one workgroup per RDM row: range-dimension CFAR at the Doppler hits and
//                  the first-argmax re-localisation (executeCFAR.m:35-89,
//                  Function_CFAR1D_sub_fixCells.m:23-87), written as a gather so the output
//                  is deterministic and needs no zero-fill pass.
//   cfar_hits*     the same as a scatter over the MTD kernel's hit lists.
//   cfar_v_kernel  the Doppler CFAR straight from an RDM (standalone rsp_cfar).
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "rsp_buf.h"
#include "rsp_internal.h"
#include "rsp_cfar_dev.h"

namespace rsp {

// ================================================================== Doppler CFAR from an RDM
// rsp_cfar's first stage: tile of W columns x V rows staged column-major in LDS.
__global__ __launch_bounds__(kBlock) void cfar_v_kernel(const float* __restrict__ rdm,
                                                        uint8_t* __restrict__ flagV, int V, int R,
                                                        int lw, CfarVArgs cv) {
    extern __shared__ __attribute__((aligned(16))) float magv[];
    const int W = 1 << lw, G = kBlock >> lw;
    const int c = threadIdx.x & (W - 1), g = threadIdx.x >> lw;
    const size_t cpi = blockIdx.y;
    const int r = blockIdx.x * W + c;
    const bool rv = r < R;
    const int ms = V + 1;
    float* mag = magv + c * ms;
    float* sums = magv + W * ms + c * ms;
    const float* src = rdm + cpi * (size_t)V * R + (rv ? r : 0);
    for (int v = g; v < V; v += G)
        mag[v] = (rv && !(v >= cv.cz_lo && v < cv.cz_hi)) ? src[(size_t)v * R] : 0.f;
    __syncthreads();
    const int run = (V + G - 1) / G;
    const int v0 = g * run, v1 = v0 + run < V ? v0 + run : V;
    doppler_sums(mag, sums, V, cv.ref, v0, v1);
    __syncthreads();
    const bool col_on = rv && in_segs(r, cv.nseg, cv.seg_lo, cv.seg_hi);
    doppler_flags(mag, sums, cv, col_on, v0, v1, flagV + cpi * (size_t)V * R + r, R, rv);
}

// log2 of the tile width: the widest of 64, 32, ... columns whose two V + 1 float columns per
// range bin fit 96 KB of LDS.
int cfar_v_tile_log2(int V) {
    int lw = 6;
    while (lw > 0 && (size_t)2 * (1 << lw) * (V + 1) * sizeof(float) > 96 * 1024) --lw;
    return lw;
}

hipError_t launch_cfar_v(const float* rdm, uint8_t* flagV, int ncpi, int V, int R,
                         const CfarVArgs& a, hipStream_t s) {
    if (ncpi <= 0) return hipSuccess;
    const int lw = cfar_v_tile_log2(V);
    const size_t lds = (size_t)2 * (1 << lw) * (V + 1) * sizeof(float);
    static LaunchOnce once;
    hipError_t e = lds_attr(once, (const void*)cfar_v_kernel, 160 * 1024);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)((R + (1 << lw) - 1) >> lw), (unsigned)ncpi), block(kBlock);
    hipLaunchKernelGGL(cfar_v_kernel, grid, block, lds, s, rdm, flagV, V, R, lw, a);
    return hipGetLastError();
}

// ================================================================== range CFAR + re-localisation
// One workgroup per RDM row.  Phase 1 stages the row (+ zero halo) and its Doppler flags in
// LDS; phase 2 forms the range window sums; phase 3 evaluates the range CFAR at every cell
// (Function_CFAR1D_sub_fixCells.m:34-58 -- the decision at a cell does not depend on which
// hit asked for it); phase 4 resolves executeCFAR.m:45-84 as a gather: cell c is flagged iff
// some Doppler hit r in {c-1, c, c+1} of c's segment picks c as the first maximum among its
// passing cells {r-1, r, r+1}.  Each thread handles 4 adjacent cells per step, so flags
// leave as coalesced 32-bit words.
constexpr int kHalo = 32;   // >= guard + ref + 2 (checked on the host)

__global__ __launch_bounds__(kBlock) void cfar_r_generic_kernel(const float* __restrict__ rdm,
                                                        const uint8_t* __restrict__ flagV,
                                                        uint8_t* __restrict__ flag, CfarRArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x;
    const int v = blockIdx.x;
    const size_t cpi = blockIdx.y;
    const int R = a.R;
    const size_t rowoff = (cpi * (size_t)a.V + v) * (size_t)R;
    uint8_t* out = flag + rowoff;
    if (v < a.lo || v >= a.hi) {
        for (int c = t; c < R; c += kBlock) out[c] = 0;
        return;
    }
    const uint8_t* fv_g = flagV + rowoff;
    if (!a.rflag) {
        for (int c = t; c < R; c += kBlock) out[c] = fv_g[c];
        return;
    }
    const int Rp = (R + 3) & ~3;                      // row length rounded to words
    const int L = Rp + 2 * kHalo;
    float* xs = reinterpret_cast<float*>(smem) + kHalo;          // xs[-kHalo, Rp + kHalo)
    float* ss = xs + L;                                            // window sums, same indexing
    uint8_t* pass = reinterpret_cast<uint8_t*>(ss - kHalo + L) + kHalo;   // pass[-kHalo, Rp+kHalo)
    uint8_t* fv = pass + L;                                        // fv[-kHalo, Rp+kHalo)
    const bool zrow = (v >= a.cz_lo && v < a.cz_hi);
    const float* xr = rdm + rowoff;
    for (int i = t; i < L; i += kBlock) {
        const int c = i - kHalo;
        const bool in = c >= 0 && c < R;
        xs[c] = (in && !zrow) ? xr[c] : 0.f;
        fv[c] = in ? fv_g[c] : 0;
        pass[c] = 0;
    }
    __syncthreads();
    const int ref = a.ref;
    for (int i = t; i < L; i += kBlock) {
        const int c = i - kHalo;
        if (c + ref > Rp + kHalo) continue;
        float s = 0.f;
        for (int k = 0; k < ref; ++k) s += xs[c + k];
        ss[c] = s;
    }
    __syncthreads();
    for (int c = t; c < R; c += kBlock) {
        int slo, shi;
        seg_of(c, a.nseg, a.seg_lo, a.seg_hi, slo, shi);
        uint8_t p = 0;
        if (shi > slo) {
            const int l1 = c - a.save - ref, r1 = c + a.save + 1;
            const bool lok = l1 >= slo, rok = r1 + ref <= shi;
            p = cfar_test(xs[c], lok ? ss[l1] : 0.f, rok ? ss[r1] : 0.f, lok, rok, a.method, a.Tr);
        }
        pass[c] = p;
    }
    __syncthreads();
    for (int c0 = 4 * t; c0 < R; c0 += 4 * kBlock) {
        // x, pass at c0-2 .. c0+5 and fv at c0-1 .. c0+4, from aligned words
        float xw[12];
        const float4 xa = *reinterpret_cast<const float4*>(xs + c0 - 4);
        const float4 xb = *reinterpret_cast<const float4*>(xs + c0);
        const float4 xc = *reinterpret_cast<const float4*>(xs + c0 + 4);
        xw[0] = xa.x; xw[1] = xa.y; xw[2] = xa.z; xw[3] = xa.w;
        xw[4] = xb.x; xw[5] = xb.y; xw[6] = xb.z; xw[7] = xb.w;
        xw[8] = xc.x; xw[9] = xc.y; xw[10] = xc.z; xw[11] = xc.w;
        const uint32_t pa = *reinterpret_cast<const uint32_t*>(pass + c0 - 4);
        const uint32_t pb = *reinterpret_cast<const uint32_t*>(pass + c0);
        const uint32_t pcw = *reinterpret_cast<const uint32_t*>(pass + c0 + 4);
        const uint32_t fa = *reinterpret_cast<const uint32_t*>(fv + c0 - 4);
        const uint32_t fb = *reinterpret_cast<const uint32_t*>(fv + c0);
        const uint32_t fc = *reinterpret_cast<const uint32_t*>(fv + c0 + 4);
        const uint64_t pw = (uint64_t)pa | ((uint64_t)pb << 32);   // byte k <-> cell c0-4+k
        const uint64_t fw = (uint64_t)fa | ((uint64_t)fb << 32);
        auto P_ = [&](int k) -> bool {   // pass at cell c0-4+k, k in [0, 12)
            return k < 8 ? ((pw >> (8 * k)) & 0xff) != 0 : ((pcw >> (8 * (k - 8))) & 0xff) != 0;
        };
        auto F_ = [&](int k) -> bool {
            return k < 8 ? ((fw >> (8 * k)) & 0xff) != 0 : ((fc >> (8 * (k - 8))) & 0xff) != 0;
        };
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j;
            int slo, shi;
            seg_of(c, a.nseg, a.seg_lo, a.seg_hi, slo, shi);
            bool f = false;
#pragma unroll
            for (int d = -1; d <= 1; ++d) {
                const int rr = c + d;   // a Doppler hit at rr tests cells rr-1 .. rr+1
                if (rr < slo || rr >= shi || !F_(4 + j + d)) continue;
                int best = -100;
                float bx = 0.f;
#pragma unroll
                for (int e = -1; e <= 1; ++e) {
                    const int q = rr + e;
                    const int k = 4 + j + d + e;
                    if (q < slo || q >= shi || !P_(k)) continue;
                    if (best == -100 || xw[k] > bx) { best = d + e; bx = xw[k]; }   // first max
                }
                f |= (best == 0);
            }
            if (c < R && f) word |= 1u << (8 * j);
        }
        if (c0 + 3 < R && (R & 3) == 0) {
            *reinterpret_cast<uint32_t*>(out + c0) = word;
        } else {
            for (int j = 0; j < 4 && c0 + j < R; ++j) out[c0 + j] = (word >> (8 * j)) & 0xff;
        }
    }
}


// Range CFAR specialised on the window (REF reference + SAVE guard cells; the reference
// uses 5 + 7): no LDS and no barriers.  Thread = 4 adjacent cells c0..c0+3 of one row; it
// reads x[c0-16, c0+20) as aligned float4s from L2 (neighbouring threads overlap in L1),
// forms the 16 window sums it needs in MATLAB's summation order, evaluates the range test
// at c0-2 .. c0+5 and resolves the four outputs as in cfar_r_generic_kernel.  Cells whose
// windows cross a segment edge take the segment-aware branch.
// Range CFAR + re-localisation for the 4 cells c0..c0+3 of one RDM row (slow path: some
// Doppler hit in c0-1..c0+4).  fa/fb/fc: flagV words of cells c0-4.., c0.., c0+4.. .
template <int REF, int SAVE>
__device__ __forceinline__ uint32_t cfar4(const float* __restrict__ xr, uint32_t fa, uint32_t fb, uint32_t fc,
                                          int c0, int R, bool zrow, const CfarRArgs& a) {
    constexpr int H = SAVE + REF + 2;          // farthest x offset a result depends on
    constexpr int B = (H + 3) & ~3;            // aligned halo
    constexpr int NX = 4 + 2 * B;              // x values held per thread
    float x[NX];   // x[k] = row[c0 - B + k]
#pragma unroll
    for (int k = 0; k < NX; k += 4) {
        const int c = c0 - B + k;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!zrow && c >= 0 && c + 3 < R) q = *reinterpret_cast<const float4*>(xr + c);
        x[k] = q.x; x[k + 1] = q.y; x[k + 2] = q.z; x[k + 3] = q.w;
    }
    int slo, shi;
    seg_of(c0, a.nseg, a.seg_lo, a.seg_hi, slo, shi);
    const bool simple = (c0 - H >= slo) && (c0 + 3 + H < shi);   // all windows inside one segment
    bool pass[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {   // cell q = c0 - 2 + i, x index B - 2 + i
        const int xi = B - 2 + i;
        float sl = 0.f, sr = 0.f;
#pragma unroll
        for (int k = 0; k < REF; ++k) sl += x[xi - SAVE - REF + k];
#pragma unroll
        for (int k = 0; k < REF; ++k) sr += x[xi + SAVE + 1 + k];
        if (simple) {
            pass[i] = x[xi] >= (a.method == 0 ? fmaxf(sl, sr) : fminf(sl, sr)) * a.Tr;
        } else {
            const int q = c0 - 2 + i;
            int ql, qh;
            seg_of(q, a.nseg, a.seg_lo, a.seg_hi, ql, qh);
            const bool lok = q - SAVE - REF >= ql, rok = q + SAVE + REF < qh;
            pass[i] = (qh > ql) && cfar_test(x[xi], sl, sr, lok, rok, a.method, a.Tr);
        }
    }
    const uint64_t fw = (uint64_t)fa | ((uint64_t)fb << 32);   // byte k <-> cell c0 - 4 + k
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + j;
        int cl = slo, ch = shi;
        if (!simple) seg_of(c, a.nseg, a.seg_lo, a.seg_hi, cl, ch);
        bool f = false;
#pragma unroll
        for (int d = -1; d <= 1; ++d) {
            const int rr = c + d;
            const int fk = 4 + j + d;
            const bool hit = fk < 8 ? ((fw >> (8 * fk)) & 0xff) != 0 : ((fc >> (8 * (fk - 8))) & 0xff) != 0;
            if (!hit || rr < cl || rr >= ch) continue;
            int best = -100;
            float bx = 0.f;
#pragma unroll
            for (int e = -1; e <= 1; ++e) {
                const int q = rr + e;
                const int i = 2 + j + d + e;   // pass/x index of cell q
                if (q < cl || q >= ch || !pass[i]) continue;
                const float xv = x[B - 2 + i];
                if (best == -100 || xv > bx) { best = d + e; bx = xv; }   // first max
            }
            f |= (best == 0);
        }
        if (f) word |= 1u << (8 * j);
    }
    return word;
}

template <int REF, int SAVE>
__global__ __launch_bounds__(kBlock) void cfar_r_kernel(const float* __restrict__ rdm,
                                                        const uint8_t* __restrict__ flagV,
                                                        uint8_t* __restrict__ flag, CfarRArgs a, int groups) {
    const int R = a.R;
    const int v = blockIdx.x / groups;
    const int c0 = ((blockIdx.x % groups) * kBlock + threadIdx.x) * 4;
    if (c0 >= R) return;
    const size_t cpi = blockIdx.y;
    const size_t rowoff = (cpi * (size_t)a.V + v) * (size_t)R;
    uint32_t* out = reinterpret_cast<uint32_t*>(flag + rowoff + c0);
    if (v < a.lo || v >= a.hi) {
        *out = 0u;
        return;
    }
    const uint32_t* fvw = reinterpret_cast<const uint32_t*>(flagV + rowoff);
    const uint32_t fa = c0 >= 4 ? fvw[c0 / 4 - 1] : 0u;
    const uint32_t fb = fvw[c0 / 4];
    const uint32_t fc = c0 + 4 < R ? fvw[c0 / 4 + 1] : 0u;
    if ((fa >> 24) == 0 && fb == 0 && (fc & 0xff) == 0) {   // no Doppler hit can reach these cells
        *out = 0u;
        return;
    }
    *out = cfar4<REF, SAVE>(rdm + rowoff, fa, fb, fc, c0, R, v >= a.cz_lo && v < a.cz_hi, a);
}

// 16 cells per thread (R % 16 == 0): one 16-B flagV load, the neighbouring groups' edge
// words from the adjacent lanes, one 16-B flag store; the 4-cell slow path runs only for
// groups with a Doppler hit within reach.  Hits are sparse, so this is the streaming pass
// over flagV -> flag at a quarter of the waves and memory instructions of cfar_r_kernel.
template <int REF, int SAVE>
__global__ __launch_bounds__(kBlock) void cfar_r16_kernel(const float* __restrict__ rdm,
                                                          const uint8_t* __restrict__ flagV,
                                                          uint8_t* __restrict__ flag, CfarRArgs a, int groups) {
    const int R = a.R;
    const int v = blockIdx.x / groups;
    const int c0 = ((blockIdx.x % groups) * kBlock + threadIdx.x) * 16;
    const bool in = c0 < R;
    const size_t cpi = blockIdx.y;
    const size_t rowoff = (cpi * (size_t)a.V + v) * (size_t)R;
    const bool row_on = v >= a.lo && v < a.hi;
    if (!in) return;
    // this group's 16 flags and the edge words of the neighbouring groups, all in one round
    // trip (the neighbours' words sit in the cache lines the adjacent lanes fetch anyway)
    uint4 f = make_uint4(0u, 0u, 0u, 0u);
    uint32_t left = 0u, right = 0u;
    if (row_on) {
        const uint8_t* fr = flagV + rowoff;
        f = *reinterpret_cast<const uint4*>(fr + c0);
        if (c0 >= 16) left = *reinterpret_cast<const uint32_t*>(fr + c0 - 4);
        if (c0 + 16 < R) right = *reinterpret_cast<const uint32_t*>(fr + c0 + 16);
    }
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    if (row_on && ((left >> 24) | f.x | f.y | f.z | f.w | (right & 0xff)) != 0) {
        const float* xr = rdm + rowoff;
        const bool zrow = v >= a.cz_lo && v < a.cz_hi;
        const uint32_t w[6] = {left, f.x, f.y, f.z, f.w, right};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint32_t fa = w[g], fb = w[g + 1], fc = w[g + 2];
            uint32_t r = 0u;
            if ((fa >> 24) != 0 || fb != 0 || (fc & 0xff) != 0) r = cfar4<REF, SAVE>(xr, fa, fb, fc, c0 + 4 * g, R, zrow, a);
            (g == 0 ? o.x : g == 1 ? o.y : g == 2 ? o.z : o.w) = r;
        }
    }
    *reinterpret_cast<uint4*>(flag + rowoff + c0) = o;
}

// Scatter form of the range stage: one thread per Doppler hit (v, r) of the MTD kernel's
// list.  Candidates q in {r-1, r, r+1} within r's column segment take the range CFAR test
// (Function_CFAR1D_sub_fixCells.m:34-58, one-sided fallback at segment edges); the first
// maximum among passing candidates gets flag 1 (executeCFAR.m:64-84).  Several hits may
// pick one cell; the writes are all 1.  Window sums are direct left-to-right adds.
// One workgroup per region (a region is one MTD workgroup's hits: up to W*P entries, ~470
// per region at c5, whose 0-v band edges fire in every column), its threads striding the list.
constexpr int kHitThreads = 256;

template <int REF, int SAVE>
__global__ __launch_bounds__(kHitThreads) void cfar_hits_kernel(const float* __restrict__ rdm,
                                                                uint8_t* __restrict__ flag,
                                                                const uint32_t* __restrict__ hits,
                                                                const uint32_t* __restrict__ counts, int nregions,
                                                                int region, CfarRArgs a) {
    cfar_hit_region<REF, SAVE>(rdm, flag, hits, counts, (int)blockIdx.x, region, a, (int)threadIdx.x, kHitThreads);
}

// The reference's window (5 reference + 7 guard cells): LPR lanes per hit region (LPR = 64: one
// wave per region, four regions per workgroup).  A region is one MTD tile's hit list (~10-50 hits
// at c3-c5), so a workgroup per region left most of its threads idle and took one dependent
// round-trip chain (count -> index -> cells) per region; here the count and the lane's first index
// load together (the index is in bounds past the count: a region holds W*P >= 256 entries), the
// lane's 17 cells follow as one batch of range-checked buffer loads (RangeJob57's gathers), and
// hits past the first LPR of a region follow in further batches the same way (the batch loop runs
// while any region of the wave has hits left, so every lane of the wave issues the gathers).
template <int LPR>
__global__ __launch_bounds__(kHitThreads) void cfar_hits57_kernel(const float* __restrict__ rdm,
                                                                  uint8_t* __restrict__ flag,
                                                                  const uint32_t* __restrict__ hits,
                                                                  const uint32_t* __restrict__ counts, int nregions,
                                                                  int region, CfarRArgs a) {
    // LPR <= 64: 64 / LPR regions per wave; LPR > 64 (a multiple of 64): a region spans LPR / 64
    // waves (the dense lists of 8192-cell regions, c5)
    constexpr int RPW = LPR >= 64 ? 1 : 64 / LPR;
    const int lane = (int)(threadIdx.x % 64);
    const int rg = LPR > 64 ? (int)(blockIdx.x * (kHitThreads / LPR) + threadIdx.x / LPR)
                            : (int)((blockIdx.x * (kHitThreads / 64) + threadIdx.x / 64) * RPW) + lane / LPR;
    if constexpr (RPW == 1) {
        if (rg >= nregions) return;   // (wave-uniform; no barriers below)
    }
    const int k = LPR > 64 ? (int)(threadIdx.x % LPR) : lane % LPR;
    constexpr int NX = RangeJob57::NX;
    const bool live = rg < nregions;
    const uint32_t* list = hits + (size_t)(live ? rg : 0) * region;
    const uint32_t n = live ? counts[rg] : 0u;
    uint32_t idx = list[k];
    const uint32_t R = (uint32_t)a.R, V = (uint32_t)a.V;
    const auto rr = buf_rsrc(rdm, kOob);
    // batches of LPR hits per region, one per lane; the next batch's index is loaded before this
    // batch's cells, so its round trip overlaps the gathers
    for (uint32_t b0 = 0;; b0 += LPR) {
        if constexpr (RPW == 1) {
            if (b0 >= n) break;
        } else {
            if (__ballot(b0 < n) == 0) break;
        }
        const bool mine = b0 + (uint32_t)k < n;
        const uint32_t nk = b0 + (uint32_t)LPR + (uint32_t)k;
        const uint32_t next = nk < n ? list[nk] : 0u;
        const uint32_t row = idx / R;
        const int r = (int)(idx - row * R);
        const int v = (int)(row % V);
        const bool zrow = v >= a.cz_lo && v < a.cz_hi;
        float x[NX];
        RangeJob57::gather(x, rr, row, r, mine && !zrow, a.R);
        if (mine) {
            int slo, shi;
            seg_of(r, a.nseg, a.seg_lo, a.seg_hi, slo, shi);
            if (shi > slo) {
                const int best = RangeJob57::test(x, r, slo, shi, a);
                if (best >= 0) flag[(size_t)row * R + best] = 1;
            }
        }
        idx = next;
    }
}

// Regions larger than 4096 cells (P = 512 tiles: c5's ~460 hits per region) take a workgroup
// each with the batched, branch-free gathers of cfar_hits57_kernel: c5 range stage 64 -> 50 us per
// 16-CPI group, +0.9 % (profiles/r05/ab/range_stage_grouping.txt).  Dev A/B: RSP_HITS_BIG=0
// restores the per-hit loads of cfar_hits_kernel.
static bool hits_big() {
    static const bool b = [] { const char* v = getenv("RSP_HITS_BIG"); return !(v && *v == '0'); }();
    return b;
}

// The kernel launch_cfar_hits runs for a list of nregions regions of `region` cells (RSP_HITS_*,
// rsp.h); *lpr: the lanes per region of the batched 5 + 7 kernel, else 0.
// (The chunk's RDM holds nregions * region cells: byte offsets stay below the range check.)
// Hits per region grow with the tile's pulse count: regions of up to 4096 cells (c3: ~10
// hits, c4: ~50) take a wave each (c4: 44 -> 31 us per launch, c3 unchanged); the 8192-cell
// regions of P = 512 (c5: ~460 hits) keep a workgroup each (a wave took 12 -> 22 us).
int cfar_hits_select(const CfarRArgs& a, int nregions, int region, int* lpr) {
    *lpr = 0;
    const bool w57 = a.ref == 5 && a.save == 7;
    const bool fits = (uint64_t)nregions * (uint64_t)region < (uint64_t)(kOob / 4u);
    if (w57 && region >= 64 && region <= 4096 && fits) {
        // lanes per region: 16 for the sparse hit lists of tiles of <= 128 Doppler rows (c3: ~11
        // hits per region, range stage 37.5 -> 29.2 us per 16-chunk group, c3 +1.3 %), a wave for
        // longer tiles (c4: ~50 hits, 46.6 us at 64 lanes against 50.1 at 32 and 56.0 at 16;
        // profiles/r05/ab/range_stage_grouping.txt).  Dev A/B: environment RSP_HITS_LPR.
        static const int lpr_env = [] { const char* v = getenv("RSP_HITS_LPR"); return v && *v ? atoi(v) : 0; }();
        const int l = lpr_env > 0 ? lpr_env : (a.V <= 128 ? 16 : 64);
        *lpr = l == 16 ? 16 : l == 32 ? 32 : 64;
        return RSP_HITS_BATCHED57;
    }
    if (w57 && region >= kHitThreads && hits_big() && fits) {
        // larger regions: the batched gathers with the whole workgroup on a region
        *lpr = kHitThreads;
        return RSP_HITS_BATCHED57;
    }
    return w57 ? RSP_HITS_PER_HIT57 : RSP_HITS_PER_HIT_RUNTIME;   // the reference's parameters / any window
}

hipError_t launch_cfar_hits(const float* rdm, uint8_t* flag, const uint32_t* hits, const uint32_t* counts,
                            int nregions, int region, const CfarRArgs& a, hipStream_t s) {
    if (nregions <= 0) return hipSuccess;
    int lpr = 0;
    const int kind = cfar_hits_select(a, nregions, region, &lpr);
    if (kind == RSP_HITS_BATCHED57 && lpr < kHitThreads) {
        auto go = [&](auto kern, int rpw) {
            const int rpb = (kHitThreads / 64) * rpw;   // regions per workgroup
            hipLaunchKernelGGL(kern, dim3((unsigned)((nregions + rpb - 1) / rpb)), dim3(kHitThreads), 0, s, rdm, flag,
                               hits, counts, nregions, region, a);
        };
        if (lpr == 16) go(cfar_hits57_kernel<16>, 4);
        else if (lpr == 32) go(cfar_hits57_kernel<32>, 2);
        else go(cfar_hits57_kernel<64>, 1);
    } else if (kind == RSP_HITS_BATCHED57) {
        hipLaunchKernelGGL(cfar_hits57_kernel<kHitThreads>, dim3((unsigned)nregions), dim3(kHitThreads), 0, s, rdm, flag,
                           hits, counts, nregions, region, a);
    } else if (kind == RSP_HITS_PER_HIT57)
        hipLaunchKernelGGL((cfar_hits_kernel<5, 7>), dim3((unsigned)nregions), dim3(kHitThreads), 0, s, rdm, flag,
                           hits, counts, nregions, region, a);
    else
        hipLaunchKernelGGL((cfar_hits_kernel<0, 0>), dim3((unsigned)nregions), dim3(kHitThreads), 0, s, rdm, flag,
                           hits, counts, nregions, region, a);
    return hipGetLastError();
}

// The window-specialised range kernels need no LDS; cfar_r_generic_kernel stages a row (+ halo)
// as x, window sums, pass and flagV bytes: 10 bytes per cell (none when rflag == 0: it copies flagV).
static bool cfar_r_specialised(const CfarRArgs& a) { return a.ref == 5 && a.save == 7 && a.rflag && (a.R & 3) == 0; }
static size_t cfar_r_generic_lds(const CfarRArgs& a) {
    return a.rflag ? (size_t)(((a.R + 3) & ~3) + 2 * kHalo) * (2 * sizeof(float) + 2) : 0;
}
bool cfar_r_supported(const CfarRArgs& a) { return cfar_r_specialised(a) || cfar_r_generic_lds(a) <= 160 * 1024; }

// The kernel launch_cfar_r runs (RSP_CFAR_R_*, rsp.h); *groups: workgroups per row of the
// window-specialised kernels (16 or 4 cells per thread), 0 for the one-workgroup-per-row kernel.
int cfar_r_select(const CfarRArgs& a, int* groups) {
    *groups = 0;
    if (cfar_r_specialised(a) && (a.R & 15) == 0) {
        *groups = (a.R / 16 + kBlock - 1) / kBlock;
        return RSP_CFAR_R_16CELL;
    }
    if (cfar_r_specialised(a)) {
        *groups = (a.R / 4 + kBlock - 1) / kBlock;
        return RSP_CFAR_R_4CELL;
    }
    return a.rflag ? RSP_CFAR_R_GENERIC : RSP_CFAR_R_COPY;   // (the copy is the generic kernel's rflag == 0 branch)
}

hipError_t launch_cfar_r(const float* rdm, const uint8_t* flagV, uint8_t* flag, int ncpi,
                         const CfarRArgs& a, hipStream_t s) {
    if (ncpi <= 0) return hipSuccess;
    if (!cfar_r_supported(a)) return hipErrorInvalidValue;
    const size_t lds = cfar_r_generic_lds(a);
    static LaunchOnce once;
    hipError_t e = lds_attr(once, (const void*)cfar_r_generic_kernel, 160 * 1024);
    if (e != hipSuccess) return e;
    int groups = 0;
    const int kind = cfar_r_select(a, &groups);
    if (kind == RSP_CFAR_R_16CELL) {   // the reference's parameters
        dim3 grid((unsigned)(groups * a.V), (unsigned)ncpi), block(kBlock);
        hipLaunchKernelGGL((cfar_r16_kernel<5, 7>), grid, block, 0, s, rdm, flagV, flag, a, groups);
        return hipGetLastError();
    }
    if (kind == RSP_CFAR_R_4CELL) {
        dim3 grid((unsigned)(groups * a.V), (unsigned)ncpi), block(kBlock);
        hipLaunchKernelGGL((cfar_r_kernel<5, 7>), grid, block, 0, s, rdm, flagV, flag, a, groups);
        return hipGetLastError();
    }
    dim3 grid((unsigned)a.V, (unsigned)ncpi), block(kBlock);
    hipLaunchKernelGGL(cfar_r_generic_kernel, grid, block, lds, s, rdm, flagV, flag, a);
    return hipGetLastError();
}

}  // namespace rsp
