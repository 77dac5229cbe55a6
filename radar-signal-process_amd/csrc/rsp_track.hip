// rsp_track.hip -- plot-to-track association from CPI to CPI for gfx950.
//
//   track_kernel   one workgroup per slot.  It loads the slot's track table into LDS, walks the
//                  batch's CPIs in order and applies to the table every CPI whose slot is its own:
//                  predict, gate, associate, update, confirm / drop, start, record (rsp.h).  The
//                  table goes back to the caller's memory once, after the walk.  Workgroup 0 also
//                  writes the outputs of the CPIs whose slot is out of range.
//
// Association.  The keys (class, cost, track, plot) are a strict total order, so the sequential
// greedy matching equals repeated rounds that match every pair which is the smallest candidate of
// both its track and its plot among the still-free ones.  A round is two scans of the free
// track x plot pairs, `lanes` lanes per track striding over the plots:
//   scan 1  a track's smallest (cost, plot), reduced over its lanes by shuffles; every in-gate pair
//           also lowers its plot's key word kc[j] = class << 63 | bits(cost) by an LDS atomic
//           minimum (a cost is a finite double >= +0, so its bits order as an integer and bit 63
//           is free for the class);
//   scan 2  the pairs that carry their plot's smallest key lower kt[j] to the smallest such track.
// A track whose own best plot answers with the track's key and index is matched.  The minima do
// not depend on the order the atomics arrive in, and every floating-point value is computed by one
// thread from LDS values: two runs give the same bytes.
// This stage is latency-bound: a few thousand pairs per round behind four barriers, on as many
// workgroups as there are slots.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/rsp.h"
#include "rsp_internal.h"

// rsp.h states every step as separate fp64 operations.  __dadd_rn, __dsub_rn and __dmul_rn are
// plain operators in this toolchain's headers, compiled under the default contraction: after
// inlining, the prediction's multiply and add came out as one v_fmac_f64.  So the operations are
// the three functions below, compiled with contraction off; the ISA has no fp64 fma.
#pragma clang fp contract(off)

namespace rsp {

namespace {

__device__ __forceinline__ double dadd(double x, double y) { return x + y; }
__device__ __forceinline__ double dsub(double x, double y) { return x - y; }
__device__ __forceinline__ double dmul(double x, double y) { return x * y; }

constexpr int kTT = 1024;         // threads of the workgroup: one per track entry at max_tracks = 1024
constexpr int kTW = kTT / 64;
constexpr size_t kTrackLdsMax = 160 * 1024 - 512;   // dynamic LDS; the rest is the static part below

// Exclusive rank of this thread among the workgroup's threads with f set, and their number.
__device__ __forceinline__ int block_rank(bool f, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(f);
    const int r = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kTW; ++i) {
        const int c = wsum[i];
        base += i < w ? c : 0;
        tot += c;
    }
    __syncthreads();   // wsum is written again by the next call
    *total = tot;
    return base + r;
}

__global__ __launch_bounds__(kTT) void track_kernel(const double* __restrict__ est, const int32_t* __restrict__ count,
                                                    int64_t batch, TrackArgs a, const int32_t* __restrict__ slot,
                                                    const double* __restrict__ dtv, double* __restrict__ state_f,
                                                    int32_t* __restrict__ state_i, int32_t* __restrict__ meta,
                                                    int32_t* __restrict__ assign, double* __restrict__ snap_f,
                                                    int32_t* __restrict__ snap_i, int32_t* __restrict__ tcount) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_wsum[kTW];
    __shared__ int s_cnt[8];   // n_valid, live, confirmed, dropped, matched
    __shared__ int s_last;     // the last round that matched a pair
    const int T = a.T, H = a.H, tid = threadIdx.x, s = blockIdx.x;
    // the table: r (the prediction between predict and update), v, ele; id, status, hist, misses,
    // hits, age, last_plot; tm = the matched plot, -1 still looking, -2 not (or no longer) looking,
    // and after the update the list of free entries
    double* tr = reinterpret_cast<double*>(smem);
    double* tv = tr + T;
    double* te = tv + T;
    // the CPI's plots: r, v; kc / kt the smallest key and its track; pa = the assign row
    double* pr = te + T;
    double* pv = pr + H;
    unsigned long long* kc = reinterpret_cast<unsigned long long*>(pv + H);
    int* ti = reinterpret_cast<int*>(kc + H);
    int* t_id = ti;
    int* t_st = ti + T;
    int* t_hist = ti + 2 * T;
    int* t_miss = ti + 3 * T;
    int* t_hits = ti + 4 * T;
    int* t_age = ti + 5 * T;
    int* t_last = ti + 6 * T;
    int* tm = ti + 7 * T;
    int* pa = tm + T;
    unsigned* kt = reinterpret_cast<unsigned*>(pa + H);

    for (int t = tid; t < T; t += kTT) {
        const double* f = state_f + ((int64_t)s * T + t) * 4;
        tr[t] = f[0];
        tv[t] = f[1];
        te[t] = f[2];
        const int32_t* q = state_i + ((int64_t)s * T + t) * 8;
#pragma unroll
        for (int k = 0; k < 7; ++k) ti[k * T + t] = q[k];
    }
    int next_id = meta[2 * s], cpis = meta[2 * s + 1];
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) s_cnt[k] = 0;
        s_last = -1;
    }
    __syncthreads();

    const unsigned mask_n = a.N >= 32 ? 0xffffffffu : (1u << a.N) - 1u;
    const int G = a.lanes, t_own = tid / G, g = tid & (G - 1);
    bool touched = false;
    int round = 0;   // counts on over the CPIs: s_last needs no reset
    for (int64_t b = 0; b < batch; ++b) {
        // everything that decides the path is the same in every thread of the workgroup
        const int sb = slot ? slot[b] : 0;
        const bool off = sb < 0 || sb >= a.slots;
        if (off ? s != 0 : sb != s) continue;
        int n = count[2 * b];
        n = n < 0 ? 0 : (n > H ? H : n);
        const double* e = est + b * (int64_t)H * 3;
        int32_t* as = assign + b * (int64_t)H;
        int32_t* tc = tcount + b * 8;
        if (off) {
            int nv = 0;
            for (int j = tid; j < H; j += kTT) {
                int v = 0;
                if (j < n) {
                    const double r = e[3 * j], vv = e[3 * j + 1];
                    const bool ok = !(r != r || vv != vv);
                    v = ok ? 0 : -1;
                    nv += ok;
                }
                as[j] = v;
            }
            if (snap_f) {
                for (int i = tid; i < 4 * T; i += kTT) snap_f[b * (int64_t)T * 4 + i] = 0.0;
                for (int i = tid; i < 8 * T; i += kTT) snap_i[b * (int64_t)T * 8 + i] = 0;
            }
            if (nv) atomicAdd(&s_cnt[0], nv);
            __syncthreads();
            if (tid == 0) {
                tc[0] = tc[1] = tc[2] = tc[3] = tc[4] = tc[6] = tc[7] = 0;
                tc[5] = s_cnt[0];
                s_cnt[0] = 0;
            }
            __syncthreads();
            continue;
        }
        touched = true;

        // ---- stage the plots, predict the tracks
        int nv = 0;
        for (int j = tid; j < n; j += kTT) {
            const double r = e[3 * j], vv = e[3 * j + 1];
            const bool ok = !(r != r || vv != vv);
            pr[j] = r;
            pv[j] = vv;
            pa[j] = ok ? 0 : -1;
            kc[j] = ~0ull;
            kt[j] = ~0u;
            nv += ok;
        }
        const double h = dtv ? dtv[b] : a.dt;
        for (int t = tid; t < T; t += kTT) {
            if (t_st[t] != 0) {
                tr[t] = dadd(tr[t], dmul(dmul(a.rate_sign, tv[t]), h));
                tm[t] = -1;
            } else {
                tm[t] = -2;
            }
        }
        __syncthreads();
        if (nv) atomicAdd(&s_cnt[0], nv);

        // ---- associate: rounds of mutual-best pairs
        for (;; ++round) {
            const bool act = t_own < T && tm[t_own] == -1;
            double bc = __longlong_as_double(0x7ff0000000000000ll), rp = 0.0, vp = 0.0;
            int bj = INT_MAX, jlo = INT_MAX, jhi = -1;
            unsigned long long cls = 0ull;
            if (act) {
                rp = tr[t_own];
                vp = tv[t_own];
                cls = t_st[t_own] == 2 ? 0ull : 1ull << 63;
                for (int j = g; j < n; j += G) {
                    if (pa[j] != 0) continue;
                    const double dr = dsub(pr[j], rp);
                    if (!(fabs(dr) <= a.gate_r)) continue;
                    const double dv = dsub(pv[j], vp);
                    if (!(fabs(dv) <= a.gate_v)) continue;
                    const double c = dadd(dmul(dmul(dr, dr), a.wr), dmul(dmul(dv, dv), a.wv));
                    atomicMin(&kc[j], cls | (unsigned long long)__double_as_longlong(c));
                    if (c < bc) {   // ascending j: a tie keeps the lower plot
                        bc = c;
                        bj = j;
                    }
                    if (jlo == INT_MAX) jlo = j;
                    jhi = j;
                }
            }
            for (int o = G >> 1; o > 0; o >>= 1) {
                const double oc = __shfl_xor(bc, o);
                const int oj = __shfl_xor(bj, o);
                if (oc < bc || (oc == bc && oj < bj)) {
                    bc = oc;
                    bj = oj;
                }
            }
            __syncthreads();
            for (int j = jlo; j <= jhi; j += G) {   // this lane's in-gate pairs lie in jlo..jhi
                if (pa[j] != 0) continue;
                const double dr = dsub(pr[j], rp);
                if (!(fabs(dr) <= a.gate_r)) continue;
                const double dv = dsub(pv[j], vp);
                if (!(fabs(dv) <= a.gate_v)) continue;
                const double c = dadd(dmul(dmul(dr, dr), a.wr), dmul(dmul(dv, dv), a.wv));
                if (kc[j] == (cls | (unsigned long long)__double_as_longlong(c))) atomicMin(&kt[j], (unsigned)t_own);
            }
            __syncthreads();
            if (act && g == 0) {
                if (bj == INT_MAX) {
                    tm[t_own] = -2;   // nothing free in its gate now, so nothing later either
                } else if (kc[bj] == (cls | (unsigned long long)__double_as_longlong(bc)) && kt[bj] == (unsigned)t_own) {
                    tm[t_own] = bj;
                    pa[bj] = t_id[t_own];
                    s_last = round;
                }
            }
            __syncthreads();
            const bool more = s_last == round;
            for (int j = tid; j < n; j += kTT)
                if (pa[j] == 0) {
                    kc[j] = ~0ull;
                    kt[j] = ~0u;
                }
            __syncthreads();
            if (!more) {
                ++round;
                break;
            }
        }

        // ---- update, confirm, drop
        int ndrop = 0, nmatch = 0;
        for (int t = tid; t < T; t += kTT) {
            int st = t_st[t];
            if (st == 0) continue;
            const int j = tm[t];
            unsigned hist = (unsigned)t_hist[t];
            int miss = t_miss[t];
            if (j >= 0) {
                const double rp = tr[t], vp = tv[t];
                tr[t] = dadd(rp, dmul(a.alpha_r, dsub(pr[j], rp)));
                tv[t] = dadd(vp, dmul(a.alpha_v, dsub(pv[j], vp)));
                const double ej = e[3 * j + 2], el = te[t];
                if (ej != ej) {
                } else if (el != el) {
                    te[t] = ej;
                } else {
                    te[t] = dadd(el, dmul(a.alpha_e, dsub(ej, el)));
                }
                hist = (hist << 1) | 1u;
                miss = 0;
                t_hits[t] = (int)((unsigned)t_hits[t] + 1u);
                t_last[t] = j;
                ++nmatch;
            } else {
                hist <<= 1;
                miss = (int)((unsigned)miss + 1u);
                t_last[t] = -1;
            }
            const int age = (int)((unsigned)t_age[t] + 1u);
            if (st == 1 && __popc(hist & mask_n) >= a.M) st = 2;
            const bool del = st == 1 ? (miss >= a.drop_t || age >= a.N) : miss >= a.drop_c;
            if (del) {
                tr[t] = tv[t] = te[t] = 0.0;
#pragma unroll
                for (int k = 0; k < 7; ++k) ti[k * T + t] = 0;
                ++ndrop;
            } else {
                t_st[t] = st;
                t_hist[t] = (int)hist;
                t_miss[t] = miss;
                t_age[t] = age;
            }
        }
        __syncthreads();

        // ---- start: the k-th unmatched valid plot takes the k-th free entry
        int nfree = 0;
        {
            const bool f = tid < T && t_st[tid] == 0;
            const int k = block_rank(f, s_wsum, &nfree);
            if (f) tm[k] = tid;   // every read of tm as the match list lies before the barrier above
        }
        int nun = 0;   // unmatched valid plots before this stretch
        for (int j0 = 0; j0 < n; j0 += kTT) {
            const int j = j0 + tid;
            const bool u = j < n && pa[j] == 0;
            int tot = 0;
            const int k = nun + block_rank(u, s_wsum, &tot);   // its first barrier also orders the list's writes
            if (u && k < nfree) {
                const int t = tm[k];
                const int id = (int)((unsigned)next_id + (unsigned)k + 1u);
                tr[t] = pr[j];
                tv[t] = pv[j];
                te[t] = e[3 * j + 2];
                t_id[t] = id;
                t_st[t] = a.M == 1 ? 2 : 1;
                t_hist[t] = 1;
                t_miss[t] = 0;
                t_hits[t] = 1;
                t_age[t] = 1;
                t_last[t] = j;
                pa[j] = id;
            }
            nun += tot;
        }
        const int started = nun < nfree ? nun : nfree;
        next_id = (int)((unsigned)next_id + (unsigned)started);
        cpis = (int)((unsigned)cpis + 1u);
        __syncthreads();

        // ---- record
        for (int j = tid; j < H; j += kTT) as[j] = j < n ? pa[j] : 0;
        int nl = 0, nc = 0;
        for (int t = tid; t < T; t += kTT) {
            nl += t_st[t] != 0;
            nc += t_st[t] == 2;
        }
        if (nl) atomicAdd(&s_cnt[1], nl);
        if (nc) atomicAdd(&s_cnt[2], nc);
        if (ndrop) atomicAdd(&s_cnt[3], ndrop);
        if (nmatch) atomicAdd(&s_cnt[4], nmatch);
        if (snap_f) {
            for (int i = tid; i < 4 * T; i += kTT) {
                const int t = i >> 2, k = i & 3;
                snap_f[b * (int64_t)T * 4 + i] = k == 0 ? tr[t] : k == 1 ? tv[t] : k == 2 ? te[t] : 0.0;
            }
            for (int i = tid; i < 8 * T; i += kTT) {
                const int t = i >> 3, k = i & 7;
                snap_i[b * (int64_t)T * 8 + i] = k < 7 ? ti[k * T + t] : 0;
            }
        }
        __syncthreads();
        if (tid == 0) {
            tc[0] = s_cnt[1];
            tc[1] = s_cnt[2];
            tc[2] = started;
            tc[3] = s_cnt[3];
            tc[4] = nun - started;
            tc[5] = s_cnt[0];
            tc[6] = s_cnt[4];
            tc[7] = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) s_cnt[k] = 0;
        }
        __syncthreads();
    }

    if (!touched) return;
    for (int i = tid; i < 4 * T; i += kTT) {
        const int t = i >> 2, k = i & 3;
        state_f[(int64_t)s * T * 4 + i] = k == 0 ? tr[t] : k == 1 ? tv[t] : k == 2 ? te[t] : 0.0;
    }
    for (int i = tid; i < 8 * T; i += kTT) {
        const int t = i >> 3, k = i & 7;
        state_i[(int64_t)s * T * 8 + i] = k < 7 ? ti[k * T + t] : 0;
    }
    if (tid == 0) {
        meta[2 * s] = next_id;
        meta[2 * s + 1] = cpis;
    }
}

LaunchOnce g_track_once;

}  // namespace

size_t track_lds_bytes(int64_t T, int64_t H) {
    // per entry three doubles and eight ints, per plot two doubles, the key word and two ints
    return (size_t)T * 56 + (size_t)H * 32;
}

size_t track_lds_max() { return kTrackLdsMax; }

int track_lanes(int T) {
    int p = 1;
    while (p < T) p <<= 1;
    const int g = kTT / p;
    return g > 64 ? 64 : (g < 1 ? 1 : g);
}

hipError_t launch_track(const double* est, const int32_t* count, int64_t batch, const TrackArgs& a0, const int32_t* slot,
                        const double* dt, double* state_f, int32_t* state_i, int32_t* meta, int32_t* assign,
                        double* snap_f, int32_t* snap_i, int32_t* tcount, hipStream_t st) {
    if (batch <= 0) return hipSuccess;
    TrackArgs a = a0;
    a.lanes = track_lanes(a.T);
    hipError_t e = lds_attr(g_track_once, (const void*)track_kernel, kTrackLdsMax);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_kernel, dim3((unsigned)a.slots), dim3(kTT), track_lds_bytes(a.T, a.H), st, est, count, batch,
                       a, slot, dt, state_f, state_i, meta, assign, snap_f, snap_i, tcount);
    return hipGetLastError();
}

}  // namespace rsp
