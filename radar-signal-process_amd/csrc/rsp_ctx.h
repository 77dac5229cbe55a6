// rsp_ctx.h -- the context behind the C ABI (private): what rsp_capi.cpp, rsp_stages.cpp and
// rsp_host.cpp share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rsp.h"
#include "rsp_hostpool.h"
#include "rsp_chunkplan.h"
#include "rsp_hostplan.h"
#include "rsp_internal.h"

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
};

struct rsp_ctx {
    int device = 0;
    bool cfar_only = false;   // created with params == NULL
    rsp_params p{};
    std::string err;
    hipStream_t stream = nullptr;
    rsp::PcArgs pc{};
    bool pc_v2 = false;                 // per-segment specialised kernels (pc_mf_kernel)
#ifndef RSP_PC_OLS_MIN
// 4096: an 8192-point segment (c4) runs as 3 blocks of 4096 points at four workgroups per CU
// instead of one whole-row transform at two: PC 289-301 -> 275-282 us per c4 step, chain +1.2-2.3 %
// (profiles/r04/ab/session9_ols4k.txt; dev-only -D for A/B of the threshold)
#define RSP_PC_OLS_MIN 4096
#endif
    int pc_ols_min = RSP_PC_OLS_MIN;    // overlap-save split of segments longer than this
    std::vector<rsp::PcMfArgs> pc_mf_whole, pc_mf_split;   // per MF segment, for rsp_set_pc_split
    std::vector<rsp::PcMfArgs> pc_mf;   // one launch per matched-filter segment
    int64_t lane_cpis[rsp::kMaxLanes] = {};   // rsp_set_lane_chunks: per-pipeline chunk sizes
    int nlane_cpis = 0;                       // 0: equal chunks / the default split
    // rsp_set_pc_prune: pruned PC kernel instances where built (dev A/B: RSP_PC_PRUNE=0 starts off)
    bool pc_prune = [] { const char* v = getenv("RSP_PC_PRUNE"); return !(v && *v == '0'); }();
    int pc_rows = 0;   // rsp_set_pc_rows: rows per long-row workgroup slot; 0: the library default
    rsp::MtdArgs mtd{};
    int64_t V = 0;                      // Doppler rows (rsp_params.mtd_nfft or P)
    int beams = 1;                      // 2: DMX left/right pair
    size_t pc_lds = 0;
    int64_t chunk = 0;  // 0 = default
    int nstreams = 0;   // chunk pipelines (the caller's stream + nstreams-1 internal ones); 0 = default
    hipStream_t aux[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    // The context's scratch (PC corner turn, hit lists, internal RDM, flagV staging) is reused by
    // every _dev call: a call's stream waits for the previous call's release event first, so
    // calls on different streams never overlap on it.
    hipEvent_t ev_scratch = nullptr;
    bool scratch_pending = false;
    std::vector<void*> owned;           // constant tables (freed at destroy)
    std::map<int, float2*> tw;          // twiddle tables by length
    DevBuf scratch_pc, tmp_flagV, tmp_rdm;
    // range concatenation between PC and MTD (rsp_set_range_concat, fun_lss_range_concate):
    // PC rows are pc_w wide (the params' R_out); the MTD and every output see p.R_out = the sum
    // of the ncat parts; cat_tmp holds the full-width PC rows of each pipeline
    int64_t pc_w = 0;
    int ncat = 0;
    int64_t cat_src[RSP_MAX_SEG] = {}, cat_len[RSP_MAX_SEG] = {};
    DevBuf cat_tmp;
    DevBuf pf_gain;                     // fused iSTC gains (rsp_set_prefilter)
    DevBuf hit_list;                    // per-lane Doppler-hit lists (fused range CFAR)
    DevBuf hit_ctr;                     // per-lane, per-MTD-workgroup hit counts
    DevBuf meas_band;                   // measurement: per-(CPI, band, column) hit counts
    DevBuf scr_ps;                      // injection: per-CPI sums, ratios and pulse phases (InjectArgs::ps)
    DevBuf cond_tmp;                    // condensation: labels, keys and hit lists of one chunk of CPIs
    DevBuf cmap_band;                   // clutter map: the band amplitudes of a call without d_band
    DevBuf integ_plan;                  // integration: where each CPI's past planes live (grow-only)
    // clutter map: window x DFT tables [P][kpad] by {P, V, window, beta bits, q_lo, q_hi, kpad} (in `owned`)
    std::map<std::vector<int64_t>, float2*> cmap_tab;
    DevBuf ing_meta;                    // ingest: per-PRT record offsets and types
    DevBuf st_in, st_canon, st_rdm, st_flag, st_flagV, st_t;  // host-API staging (rsp_cfar)
    // Pipelined host-buffer path (rsp_pc_mtd_cfar / rsp_pc_mtd): chunk k's H2D (copy stream),
    // chain (ctx->stream) and D2H (copy stream) overlap chunks k+1 and k-1; pageable <-> pinned
    // staging through rings of pinned pieces, copied by a host thread pool.
    struct HostPipe {
        static constexpr int kSlots = 2;      // chunk slots (device buffers)
        static constexpr int kRing = 4;       // pinned pieces per direction
        hipStream_t s_h2d = nullptr, s_d2h = nullptr;
        DevBuf in[kSlots], canon[kSlots], rdm[kSlots], flag[kSlots], flagV[kSlots], tr[kSlots][3];
        hipEvent_t ev_in[kSlots] = {}, ev_comp[kSlots] = {}, ev_out[kSlots] = {};
        void* pin_in[kRing] = {};
        void* pin_out[kRing] = {};
        hipEvent_t ev_pin_in[kRing] = {}, ev_pin_out[kRing] = {};
        size_t piece = 0;                     // bytes per pinned piece
        int ring_in = 0;                      // next input piece slot
        int threads = 0;                      // requested copy threads (0 = default)
        std::unique_ptr<rsp::CopyPool> pool;
        std::unique_ptr<rsp::Prefaulter> prefault;   // fresh output arrays (host_prefault)
        rsp::Prefaulter* pf = nullptr;                // the running call's prefault job, if any
        // one-chunk calls (host_chain_small): pinned staging the kernels read and write directly
        static constexpr int kParts = rsp::kParts;   // output parts in flight (one event each)
        void* zc_in = nullptr;
        void* zc_out = nullptr;
        size_t zc_in_n = 0, zc_out_n = 0;
        hipEvent_t ev_part[kParts] = {};
    } hp;
    int64_t host_chunk = 0;                   // CPIs per host chunk (0 = by bytes)
    // diagnostics (rsp_profile): HIP event pairs around each kernel launch
    struct Ev {
        int k;
        hipEvent_t a, b;
    };
    int prof = 0;            // 0 off; N >= 1: bracket every N-th launch
    uint64_t prof_tick = 0;
    std::vector<Ev> evs;
    size_t nev = 0;
    double prof_ms[RSP_NKERNELS] = {};
    int64_t prof_n[RSP_NKERNELS] = {};
};

// defined in rsp_capi.cpp
int fail(rsp_ctx* ctx, int code, const char* fmt, ...);
int ensure(rsp_ctx* ctx, DevBuf& b, size_t bytes);
bool set_device(rsp_ctx* ctx);
namespace rsp {
// Order this call's use of the context scratch after the previous call's (on any stream).
int scratch_acquire(rsp_ctx* ctx, hipStream_t s);
int scratch_release(rsp_ctx* ctx, hipStream_t s);
// Window of n points (RSP_WIN_*) in fp64.
std::vector<double> make_window(int kind, double beta, int64_t n);
}  // namespace rsp

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail((ctx), RSP_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                                 \
    } while (0)

namespace rsp {
// A host table into device memory the context owns (freed at destroy).
template <typename T>
int upload(rsp_ctx* ctx, const std::vector<T>& h, T** out) {
    void* d = nullptr;
    HIP_TRY(ctx, hipMalloc(&d, h.size() * sizeof(T)));
    ctx->owned.push_back(d);
    HIP_TRY(ctx, hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (T*)d;
    return RSP_OK;
}
}  // namespace rsp
