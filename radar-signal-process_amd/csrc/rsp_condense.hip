// rsp_condense.hip -- plot condensation for gfx950: the CFAR hits of a V x R
// window are labelled into connected components (adjacent: row distance <= gap_v, optionally
// around the Doppler seam, and column distance <= gap_r) and each component ("plot") keeps its
// strongest cell.  Outputs: a flag plane with only the peaks set, which the measurement
// (rsp_measure.hip) accepts as it stands, one 8-int record per plot in the measurement's hit
// order, and the counts.
//
// The work per CPI, seven launches over a chunk of CPIs:
//   cond_list_kernel   the only dense pass: a thread reads 16 flag bytes in each of four rows and
//                      writes as many zero bytes of the peak plane; every hit gets a slot of the CPI's hit list
//                      (one integer add per wave on the CPI's counter), its own label
//                      L[cell] = cell and an empty peak key K[cell] = 0.  L and K are cell-indexed
//                      planes that are written and read at flagged cells only: nothing sweeps them.
//   cond_union_kernel  one thread per listed hit: for each flagged cell in the forward half of
//                      its neighbourhood (sparse byte reads of the flag plane), unite the two
//                      label trees -- find both roots, atomicMin the larger root's label to the
//                      smaller; a root someone else moved first is followed and the step
//                      repeated.  Labels only decrease, so every loop ends; no thread waits for
//                      another thread's store.
//   cond_root_kernel   per hit: its root (the label is flattened to it) and an atomicMax of the
//                      hit's 64-bit key (amplitude bits << 32 | ~(r*V + v)) on K[root].
//   cond_peak_kernel   per hit: the one whose cell is in K[root] sets its byte of the peak plane.
//   hits_kernel        (rsp_measure.hip, unchanged) lists the peak plane's hits in find() order:
//                      the plot order, and the plot count.
//   cond_emit_kernel   per listed peak: the record's fixed fields, and K[root] = plot index.
//   cond_accum_kernel  per hit: n_cells and the bounding box of its plot by integer add / min / max.
// Every combination across threads is an integer atomic whose result does not depend on the
// order of arrival (min, max, add), and the order of the hit list -- the one thing that does
// depend on scheduling -- reaches no output.  So two runs give the same bytes, and a CPI gives
// the same bytes alone as in a batch.
//
// Amplitudes at flagged cells are magnitudes; where one is negative or NaN its bit pattern does
// not order as its value and the choice of peak is unspecified (-0 counts as 0).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsp.h"
#include "rsp_internal.h"

namespace rsp {

namespace {

constexpr int kT = 256;
typedef unsigned long long u64;

__device__ __forceinline__ int ld_label(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int find_root(const int32_t* L, int a) {
    int p = ld_label(L + a);
    while (p != a) {
        a = p;
        p = ld_label(L + a);
    }
    return a;
}

// Labels only decrease and a label always names a cell of the same component, so a stale read
// is an earlier valid state: the atomicMin tells whether `a` was still a root, and if not the
// loop goes on from the label found there, which is smaller.
__device__ void unite(int32_t* L, int a, int b) {
    for (;;) {
        const int a0 = a, b0 = b;
        a = find_root(L, a);
        b = find_root(L, b);
        // shorten the paths walked (a root is a smaller label of the same component)
        if (a != a0) atomicMin(L + a0, a);
        if (b != b0) atomicMin(L + b0, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

// The dense pass.  A workgroup owns a tile of kRowsPerThread * 256 / tw rows x tw 16-byte granules;
// a thread owns one granule in each of kRowsPerThread rows, so that its loads are in flight
// together.  ALIGNED (the flag and peak windows share their address modulo 16, the usual case:
// same geometry, allocator-aligned planes): the granules are the memory's own 16-byte lines, read
// with one aligned load each whatever the window's column and pitch; bytes of a line outside the
// window's columns are masked off and never written (an aligned 16-byte load that holds one byte
// of the plane lies inside the plane's pages).  Otherwise granule g is columns 16g.. of the row,
// read and written byte by byte.
constexpr int kRowsPerThread = 4;

template <bool ALIGNED>
__global__ __launch_bounds__(kT) void cond_list_kernel(const uint8_t* __restrict__ flag, uint8_t* __restrict__ peak,
                                                       CondenseArgs a, int32_t* __restrict__ L, u64* __restrict__ K,
                                                       int32_t* __restrict__ list, int32_t* __restrict__ nhits) {
    const int cpi = blockIdx.y;
    const int tw = a.tw, tr = kT / tw;
    const int S = (a.R + (ALIGNED ? 30 : 15)) >> 4;   // granules a row can touch
    const int tiles_x = (S + tw - 1) / tw;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int seg = tx * tw + (int)threadIdx.x % tw;
    const int v_first = ty * tr * kRowsPerThread + (int)threadIdx.x / tw;
    uint32_t pat[kRowsPerThread];
    int c_lo[kRowsPerThread];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int v = v_first + k * tr;
        pat[k] = 0;
        c_lo[k] = 0;
        if (v >= a.V) continue;
        const size_t row = (size_t)cpi * a.cs + (size_t)v * a.ld;
        const uint8_t* p = flag + row;
        const int sh = ALIGNED ? (int)((uintptr_t)p & 15) : 0;
        const int lo = seg * 16 - sh;                            // window column of the granule's byte 0
        const int j0 = max(0, -lo), j1 = min(16, a.R - lo);      // its bytes inside the window
        c_lo[k] = lo;
        if (j0 >= j1) continue;
        uint8_t* q = peak + row;
        if constexpr (ALIGNED) {
            const uint4 w = *reinterpret_cast<const uint4*>(p + lo);
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
            uint32_t bits = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // high bit of each byte = byte nonzero
                const uint32_t t = (((ws[i] & 0x7f7f7f7fu) + 0x7f7f7f7fu) | ws[i]) & 0x80808080u;
                bits |= (((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u)) << (4 * i);
            }
            pat[k] = bits & ((1u << j1) - 1u) & ~((1u << j0) - 1u);
            if (j1 - j0 == 16) {
                *reinterpret_cast<uint4*>(q + lo) = make_uint4(0, 0, 0, 0);
            } else {
                for (int j = j0; j < j1; ++j) q[lo + j] = 0;
            }
        } else {
            for (int j = j0; j < j1; ++j) {
                pat[k] |= (p[lo + j] ? 1u : 0u) << j;
                q[lo + j] = 0;
            }
        }
        cnt += __popc(pat[k]);
    }
    // slots: the wave's hits take one range of the CPI's list
    const int lane = threadIdx.x & 63;
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    int base = 0;
    if (lane == 63 && inc) base = atomicAdd(nhits + cpi, inc);
    base = __shfl(base, 63, 64);
    int slot = base + inc - cnt;
    int32_t* Lc = L + (size_t)cpi * a.cells;
    u64* Kc = K + (size_t)cpi * a.cells;
    int32_t* lc = list + (size_t)cpi * a.cells;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        uint32_t m = pat[k];
        while (m) {
            const int j = __builtin_ctz(m);
            m &= m - 1;
            const int idx = (v_first + k * tr) * a.R + c_lo[k] + j;
            lc[slot++] = idx;
            Lc[idx] = idx;
            Kc[idx] = 0;
        }
    }
}

__global__ __launch_bounds__(kT) void cond_union_kernel(const uint8_t* __restrict__ flag, CondenseArgs a,
                                                        int32_t* __restrict__ L, const int32_t* __restrict__ list,
                                                        const int32_t* __restrict__ nhits) {
    const int cpi = blockIdx.y;
    const int n = nhits[cpi];
    const uint8_t* fl = flag + (size_t)cpi * a.cs;
    int32_t* Lc = L + (size_t)cpi * a.cells;
    const int32_t* lc = list + (size_t)cpi * a.cells;
    for (int h = blockIdx.x * kT + threadIdx.x; h < n; h += gridDim.x * kT) {
        const int idx = lc[h];
        const int v = idx / a.R, c = idx - v * a.R;
        // the forward half of the neighbourhood: the other half unites from its own side
        for (int dc = 0; dc <= a.gap_r; ++dc) {
            const int c2 = c + dc;
            if (c2 >= a.R) break;
            for (int dv = dc ? -a.gap_v : 1; dv <= a.gap_v; ++dv) {
                int v2 = v + dv;
                if (a.wrap_v) {
                    v2 = v2 < 0 ? v2 + a.V : (v2 >= a.V ? v2 - a.V : v2);
                } else if (v2 < 0 || v2 >= a.V) {
                    continue;
                }
                if (fl[(size_t)v2 * a.ld + c2]) unite(Lc, idx, v2 * a.R + c2);
            }
        }
    }
}

__global__ __launch_bounds__(kT) void cond_root_kernel(const float* __restrict__ amp, CondenseArgs a,
                                                       int32_t* __restrict__ L, u64* __restrict__ K,
                                                       const int32_t* __restrict__ list,
                                                       const int32_t* __restrict__ nhits) {
    const int cpi = blockIdx.y;
    const int n = nhits[cpi];
    const float* am = amp + (size_t)cpi * a.cs;
    int32_t* Lc = L + (size_t)cpi * a.cells;
    u64* Kc = K + (size_t)cpi * a.cells;
    const int32_t* lc = list + (size_t)cpi * a.cells;
    for (int h = blockIdx.x * kT + threadIdx.x; h < n; h += gridDim.x * kT) {
        const int idx = lc[h];
        const int v = idx / a.R, c = idx - v * a.R;
        const float x = am[(size_t)v * a.ld + c];
        const int r = find_root(Lc, idx);
        // flatten: no union runs in this launch, so a reader finds the old label or the root
        if (r != idx) __hip_atomic_store(Lc + idx, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t bits = x == 0.0f ? 0u : __float_as_uint(x);
        const u64 key = ((u64)bits << 32) | (uint32_t)~(uint32_t)(c * a.V + v);
        // K[root] only grows: a stale smaller value costs an atomic, never a wrong skip
        if (__hip_atomic_load(Kc + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(Kc + r, key);
    }
}

__global__ __launch_bounds__(kT) void cond_peak_kernel(uint8_t* __restrict__ peak, CondenseArgs a,
                                                       const int32_t* __restrict__ L, const u64* __restrict__ K,
                                                       const int32_t* __restrict__ list,
                                                       const int32_t* __restrict__ nhits) {
    const int cpi = blockIdx.y;
    const int n = nhits[cpi];
    uint8_t* pk = peak + (size_t)cpi * a.cs;
    const int32_t* Lc = L + (size_t)cpi * a.cells;
    const u64* Kc = K + (size_t)cpi * a.cells;
    const int32_t* lc = list + (size_t)cpi * a.cells;
    for (int h = blockIdx.x * kT + threadIdx.x; h < n; h += gridDim.x * kT) {
        const int idx = lc[h];
        const int v = idx / a.R, c = idx - v * a.R;
        const u64 key = Kc[Lc[idx]];
        if ((uint32_t)~(uint32_t)key == (uint32_t)(c * a.V + v)) pk[(size_t)v * a.ld + c] = 1;
    }
}

// pl: the peak plane's hit list (hits_kernel: cell v*R + c in the first of three words per slot,
// list_cap slots per CPI),
// pcount its {count, -}.  K[root] becomes the plot's index, told apart from a key by bits 31..63
// (a key's low word is ~(r*V + v) with r*V + v < 2^31).
__global__ __launch_bounds__(kT) void cond_emit_kernel(CondenseArgs a, const int32_t* __restrict__ L,
                                                       u64* __restrict__ K, const int64_t* __restrict__ pl,
                                                       const int32_t* __restrict__ pcount,
                                                       const int32_t* __restrict__ nhits, int32_t* __restrict__ plots,
                                                       int32_t* __restrict__ count) {
    const int cpi = blockIdx.y;
    const int np = pcount[cpi * 2];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        count[cpi * 2 + 0] = np;
        count[cpi * 2 + 1] = nhits[cpi];
    }
    if (!plots) return;
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= np || i >= a.max_plots) return;
    const int64_t cell = pl[((size_t)cpi * a.list_cap + i) * 3];
    const int v = (int)(cell / a.R), c = (int)(cell - (int64_t)v * a.R);
    const int r = L[(size_t)cpi * a.cells + (size_t)v * a.R + c];
    K[(size_t)cpi * a.cells + r] = (u64)i;
    int32_t* rec = plots + ((size_t)cpi * a.max_plots + i) * 8;
    rec[0] = v;
    rec[1] = c;
    rec[2] = 0;
    rec[3] = v;   // the box starts at the peak cell: a one-cell plot then needs no min / max at all
    rec[4] = v;
    rec[5] = c;
    rec[6] = c;
    rec[7] = 0;
}

__device__ __forceinline__ void min_to(int32_t* p, int x) {
    if (x < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, x);
}
__device__ __forceinline__ void max_to(int32_t* p, int x) {
    if (x > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, x);
}

__global__ __launch_bounds__(kT) void cond_accum_kernel(CondenseArgs a, const int32_t* __restrict__ L,
                                                        const u64* __restrict__ K, const int32_t* __restrict__ list,
                                                        const int32_t* __restrict__ nhits,
                                                        int32_t* __restrict__ plots) {
    const int cpi = blockIdx.y;
    const int n = nhits[cpi];
    const int32_t* Lc = L + (size_t)cpi * a.cells;
    const u64* Kc = K + (size_t)cpi * a.cells;
    const int32_t* lc = list + (size_t)cpi * a.cells;
    for (int h = blockIdx.x * kT + threadIdx.x; h < n; h += gridDim.x * kT) {
        const int idx = lc[h];
        const int v = idx / a.R, c = idx - v * a.R;
        const u64 k = Kc[Lc[idx]];
        if (k >> 31) continue;   // still a key: a plot past max_plots, counted but not written
        int32_t* rec = plots + ((size_t)cpi * a.max_plots + (int)k) * 8;
        // a wave whose active lanes all belong to one plot (the common case inside a large
        // plot) adds its lane count once
        const int k0 = __shfl((int)k, __builtin_ctzll(__ballot(1)), 64);
        const uint64_t same = __ballot((int)k == k0), act = __ballot(1);
        if (same == act) {
            if ((int)(threadIdx.x & 63) == __builtin_ctzll(act)) atomicAdd(rec + 2, __popcll(act));
        } else {
            atomicAdd(rec + 2, 1);
        }
        min_to(rec + 3, v);
        max_to(rec + 4, v);
        min_to(rec + 5, c);
        max_to(rec + 6, c);
    }
}

}  // namespace

size_t condense_scratch_per_cpi(int64_t V, int64_t R, int32_t max_plots) {
    const size_t cells = (size_t)V * (size_t)R;
    const size_t np = (size_t)max_plots < cells ? (size_t)max_plots : cells;
    // labels 4 B, keys 8 B, hit list 4 B per cell; the peaks' list (3 x 8 B per slot); 3 counters
    size_t n = cells * 16 + np * 24 + 16;
    return (n + 15) & ~(size_t)15;
}

// One chunk of `batch` CPIs; scratch: condense_scratch_per_cpi() * batch bytes, 16-byte aligned.
hipError_t launch_condense(const float* amp, const uint8_t* flag, uint8_t* peak, int batch, CondenseArgs a,
                           int32_t* plots, int32_t* count, void* scratch, hipStream_t st) {
    if (batch <= 0) return hipSuccess;
    const size_t cells = a.cells, nb = (size_t)batch;
    if (!plots) a.max_plots = 0;   // as condense_scratch_per_cpi was asked: no peaks' list
    const size_t np = (size_t)a.max_plots < cells ? (size_t)a.max_plots : cells;
    char* s = (char*)scratch;
    u64* K = (u64*)s;
    s += nb * cells * 8;
    int64_t* pl = (int64_t*)s;
    s += nb * np * 24;
    int32_t* L = (int32_t*)s;
    s += nb * cells * 4;
    int32_t* list = (int32_t*)s;
    s += nb * cells * 4;
    int32_t* nhits = (int32_t*)s;
    s += nb * 4;
    int32_t* pcount = (int32_t*)s;
    a.list_cap =a.max_plots ? (int)np : 0;   // a window holds at most `cells` plots
    hipError_t err = hipMemsetAsync(nhits, 0, nb * 4, st);
    if (err != hipSuccess) return err;
    const bool aligned = (((uintptr_t)flag ^ (uintptr_t)peak) & 15) == 0;
    const int S = (a.R + (aligned ? 30 : 15)) / 16;
    a.tw = 1;
    while (a.tw < S && a.tw < 16) a.tw <<= 1;
    const int tr = kT / a.tw * kRowsPerThread;
    const int64_t tiles = (int64_t)((S + a.tw - 1) / a.tw) * ((a.V + tr - 1) / tr);
    if (tiles > 0x7fffffff || batch > 65535) return hipErrorInvalidConfiguration;
    if (aligned)
        hipLaunchKernelGGL(cond_list_kernel<true>, dim3((unsigned)tiles, batch), dim3(kT), 0, st, flag, peak, a, L, K, list,
                           nhits);
    else
        hipLaunchKernelGGL(cond_list_kernel<false>, dim3((unsigned)tiles, batch), dim3(kT), 0, st, flag, peak, a, L, K, list,
                           nhits);
    // hits are sparse: a few workgroups per CPI stride over its list
    const size_t want = (cells + kT - 1) / kT;
    const unsigned nbx = (unsigned)(want < 64 ? want : 64);
    hipLaunchKernelGGL(cond_union_kernel, dim3(nbx, batch), dim3(kT), 0, st, flag, a, L, list, nhits);
    hipLaunchKernelGGL(cond_root_kernel, dim3(nbx, batch), dim3(kT), 0, st, amp, a, L, K, list, nhits);
    hipLaunchKernelGGL(cond_peak_kernel, dim3(nbx, batch), dim3(kT), 0, st, peak, a, L, K, list, nhits);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    err = launch_hit_list(peak, a.V, a.R, batch, a.ld, a.cs, a.list_cap, pl, pcount, st);
    if (err != hipSuccess) return err;
    const unsigned nbe = a.max_plots > 0 ? (unsigned)((np + kT - 1) / kT) : 1u;
    hipLaunchKernelGGL(cond_emit_kernel, dim3(nbe ? nbe : 1u, batch), dim3(kT), 0, st, a, L, K, pl, pcount, nhits,
                       a.max_plots > 0 ? plots : nullptr, count);
    if (a.max_plots > 0)
        hipLaunchKernelGGL(cond_accum_kernel, dim3(nbx, batch), dim3(kT), 0, st, a, L, K, list, nhits, plots);
    return hipGetLastError();
}

}  // namespace rsp
