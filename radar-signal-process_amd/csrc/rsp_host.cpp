// rsp_host.cpp -- the host-buffer entry points of the C ABI (include/rsp.h), on top of the
// device entry points (rsp_pc_mtd_cfar_dev, rsp_cfar_dev) of rsp_capi.cpp.  Three routes:
//   * the chunked DMA pipeline (host_chain, cfar_f64_body's second half): chunk k's H2D, chain
//     and D2H overlap chunks k+1 and k-1 through rings of pinned pieces filled and emptied by the
//     copy threads.  rsp_pc_mtd_cfar, rsp_pc_mtd_cfar_f64 and rsp_pc_mtd with more than one host
//     chunk, and rsp_cfar_f64 beyond the one-chunk limits;
//   * the one-chunk pinned path (host_chain_small, cfar_f64_body's first half): kernels read the
//     input from, and write the outputs into, coherent pinned staging piece by piece.  The same
//     four entry points when the call is one chunk and zc_eligible() (MATLAB's one CPI per call);
//   * rsp_cfar's plain route: one synchronous hipMemcpyAsync each way, no copy threads -- kept
//     apart as the independent form the tests compare rsp_cfar_f64 against.
// All piece / part / chunk arithmetic is rsp_hostplan.h's; this file loops over its lists.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <new>
#include <thread>
#include <utility>
#include <vector>

#include "rsp_ctx.h"

using rsp::Conv;

static size_t dtype_size(int32_t dtype) {   // 0: no such dtype
    return dtype == RSP_C64 ? 8 : (dtype == RSP_C128 ? 16 : (dtype == RSP_C32F16 ? 4 : 0));
}

template <typename T>
static int fetch(rsp_ctx* ctx, const T* d, T* h, int64_t batch, int64_t A, int64_t B, int32_t layout) {
    const size_t n = (size_t)batch * A * B;
    if (layout == RSP_COLMAJOR) {
        int rc = ensure(ctx, ctx->st_t, n * sizeof(T));
        if (rc) return rc;
        hipError_t e;
        if (sizeof(T) == 4)
            e = rsp::launch_transpose_f32((const float*)d, (float*)ctx->st_t.p, batch, (int)A, (int)B, ctx->stream);
        else
            e = rsp::launch_transpose_u8((const uint8_t*)d, (uint8_t*)ctx->st_t.p, batch, (int)A, (int)B, ctx->stream);
        HIP_TRY(ctx, e);
        d = (const T*)ctx->st_t.p;
    }
    HIP_TRY(ctx, hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RSP_OK;
}

static int check_host_call(rsp_ctx* ctx, const void* echo, int32_t dtype, int32_t layout, int64_t P,
                           int64_t R, int64_t batch) {
    if (ctx->cfar_only) return fail(ctx, RSP_ERR_ARG, "context was created for CFAR only (params == NULL)");
    if (!echo || batch < 0) return fail(ctx, RSP_ERR_ARG, "null echo or negative batch");
    if (!dtype_size(dtype)) return fail(ctx, RSP_ERR_ARG, "bad dtype %d", dtype);
    if (layout != RSP_ROWMAJOR && layout != RSP_COLMAJOR) return fail(ctx, RSP_ERR_ARG, "bad layout %d", layout);
    if (P != ctx->p.P || R != ctx->p.R)
        return fail(ctx, RSP_ERR_SHAPE, "echo is %lld x %lld but the context was created for %lld x %lld",
                    (long long)P, (long long)R, (long long)ctx->p.P, (long long)ctx->p.R);
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    return RSP_OK;
}

// Dev-only A/B knobs of this file (environment, read once per process).
struct HostKnobs {
    int zc;                   // RSP_HOST_ZC: 0 the DMA pipeline for every call, 1 coherent staging, 2 non-coherent
    size_t part, piece;       // RSP_ZC_PART_KIB / RSP_ZC_PIECE_KIB: one-chunk output part / input piece bytes
    int prefault, prefault_threads, prefault_huge;   // RSP_PREFAULT=0 off, _THREADS, _HUGE=0 no MADV_HUGEPAGE advice
    bool trace;               // RSP_HOST_TRACE=1: HostTrace
};
static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}
static const HostKnobs& knobs() {
    static const HostKnobs k = {env_int("RSP_HOST_ZC", 1), (size_t)env_int("RSP_ZC_PART_KIB", rsp::kZcPart >> 10) << 10,
                                (size_t)env_int("RSP_ZC_PIECE_KIB", rsp::kZcPiece >> 10) << 10, env_int("RSP_PREFAULT", 1),
                                env_int("RSP_PREFAULT_THREADS", 4), env_int("RSP_PREFAULT_HUGE", 1),
                                env_int("RSP_HOST_TRACE", 0) == 1};
    return k;
}

// ---- pipelined host path
static int host_pipe_init(rsp_ctx* ctx) {
    auto& h = ctx->hp;
    if (h.s_h2d) return RSP_OK;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&h.s_h2d, hipStreamNonBlocking));
    HIP_TRY(ctx, hipStreamCreateWithFlags(&h.s_d2h, hipStreamNonBlocking));
    for (int i = 0; i < h.kSlots; ++i) {
        HIP_TRY(ctx, hipEventCreateWithFlags(&h.ev_in[i], hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&h.ev_comp[i], hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&h.ev_out[i], hipEventDisableTiming));
    }
    for (auto& e : h.ev_part) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    h.piece = rsp::kHostPiece;
    for (int i = 0; i < h.kRing; ++i) {
        HIP_TRY(ctx, hipHostMalloc(&h.pin_in[i], h.piece, hipHostMallocDefault));
        HIP_TRY(ctx, hipHostMalloc(&h.pin_out[i], h.piece, hipHostMallocDefault));
        HIP_TRY(ctx, hipEventCreateWithFlags(&h.ev_pin_in[i], hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&h.ev_pin_out[i], hipEventDisableTiming));
    }
    return RSP_OK;
}

// (thread creation can throw: callers run inside drained(), which turns any exception into an
// error status -- nothing may unwind through the extern "C" boundary into the MEX host)
static rsp::CopyPool& host_pool(rsp_ctx* ctx) {
    auto& h = ctx->hp;
    int want = h.threads;
    if (want <= 0) {
        const unsigned hc = std::thread::hardware_concurrency();
        want = hc >= 16 ? 8 : (hc >= 4 ? (int)hc / 2 : 1);
    }
    if (!h.pool || h.pool->threads() != want) {
        h.pool.reset();
        h.pool.reset(new rsp::CopyPool(want));
    }
    return *h.pool;
}

// The copy threads' work on `dev_bytes` device-side bytes: a copy, MATLAB's complex double or
// double narrowed to float on the way in (the same round-to-nearest cast the device conversion
// does, at half the PCIe bytes), or float cells / 0-1 bytes widened to MATLAB's double on the
// way out.  The host side is at conv_host_bytes() of the device-side offset.
static void convert(rsp::CopyPool& pool, Conv c, void* dst, const void* src, size_t dev_bytes) {
    switch (c) {
        case Conv::kNone: pool.copy(dst, src, dev_bytes); break;
        case Conv::kC128toC64: pool.narrow_c128((float*)dst, (const double*)src, dev_bytes / 8); break;
        case Conv::kF64toF32: pool.narrow_f64((float*)dst, (const double*)src, dev_bytes / 4); break;
        case Conv::kF32toF64: pool.widen_f32((double*)dst, (const float*)src, dev_bytes / 4); break;
        case Conv::kU8toF64: pool.widen_u8((double*)dst, (const uint8_t*)src, dev_bytes); break;
    }
}

// host (pageable) -> device, through the pinned input ring on the H2D stream: piece i is
// converted into a ring slot by the pool while the DMA of piece i-1 runs.  `bytes` = device side.
static int h2d_pieces(rsp_ctx* ctx, void* d, const void* src, size_t bytes, Conv conv) {
    auto& h = ctx->hp;
    rsp::CopyPool& pool = host_pool(ctx);
    const size_t piece = rsp::piece_for(bytes, h.piece);
    for (size_t off = 0; off < bytes; off += piece) {
        const size_t n = bytes - off < piece ? bytes - off : piece;
        const int r = h.ring_in;
        h.ring_in = (h.ring_in + 1) % h.kRing;
        HIP_TRY(ctx, hipEventSynchronize(h.ev_pin_in[r]));   // the slot's previous DMA is done
        convert(pool, conv, h.pin_in[r], (const char*)src + rsp::conv_host_bytes(conv, off), n);
        HIP_TRY(ctx, hipMemcpyAsync((char*)d + off, h.pin_in[r], n, hipMemcpyHostToDevice, h.s_h2d));
        HIP_TRY(ctx, hipEventRecord(h.ev_pin_in[r], h.s_h2d));
    }
    return RSP_OK;
}

// device -> host (pageable), through the pinned output ring on the D2H stream: up to kRing
// pieces in flight; each is converted out by the pool once its DMA is done (bytes = device side).
struct D2HPart {
    const void* d;
    void* h;
    size_t bytes;
    Conv conv;
};
static int d2h_pieces(rsp_ctx* ctx, const std::vector<D2HPart>& parts) {
    auto& h = ctx->hp;
    rsp::CopyPool& pool = host_pool(ctx);
    std::vector<D2HPart> ps;
    for (const D2HPart& p : parts) {
        const size_t piece = rsp::piece_for(p.bytes, h.piece);
        for (size_t off = 0; off < p.bytes; off += piece)
            ps.push_back({(const char*)p.d + off, (char*)p.h + rsp::conv_host_bytes(p.conv, off),
                          p.bytes - off < piece ? p.bytes - off : piece, p.conv});
    }
    const size_t np = ps.size();
    auto issue = [&](size_t i) -> int {
        const int r = (int)(i % h.kRing);
        HIP_TRY(ctx, hipMemcpyAsync(h.pin_out[r], ps[i].d, ps[i].bytes, hipMemcpyDeviceToHost, h.s_d2h));
        HIP_TRY(ctx, hipEventRecord(h.ev_pin_out[r], h.s_d2h));
        return RSP_OK;
    };
    int rc;
    for (size_t i = 0; i < np && i < (size_t)h.kRing; ++i)
        if ((rc = issue(i))) return rc;
    for (size_t i = 0; i < np; ++i) {
        const int r = (int)(i % h.kRing);
        HIP_TRY(ctx, hipEventSynchronize(h.ev_pin_out[r]));
        if (h.pf) h.pf->wait(ps[i].h, rsp::conv_host_bytes(ps[i].conv, ps[i].bytes));
        convert(pool, ps[i].conv, ps[i].h, h.pin_out[r], ps[i].bytes);
        if (i + h.kRing < np && (rc = issue(i + h.kRing))) return rc;
    }
    return RSP_OK;
}

int rsp_set_host_pipeline(rsp_ctx* ctx, int64_t cpis_per_chunk, int32_t copy_threads) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "null ctx");
    if (cpis_per_chunk < 0 || copy_threads < 0 || copy_threads > 64)
        return fail(ctx, RSP_ERR_ARG, "rsp_set_host_pipeline: chunk %lld, threads %d", (long long)cpis_per_chunk,
                    (int)copy_threads);
    ctx->host_chunk = cpis_per_chunk;
    ctx->hp.threads = copy_threads;
    return RSP_OK;
}

// Runs an entry point's body: any exception becomes an error status, and after an error once
// chunks may have been issued all three streams are drained before returning, so the next
// call's first H2D cannot overwrite an input slot a chain still reads, nor its output staging
// race a D2H still in flight (the status stays the first error's).
template <typename F>
static int drained(rsp_ctx* ctx, const char* fn, F&& body) {
    int rc;
    try {
        rc = body();
    } catch (const std::bad_alloc&) {
        rc = fail(ctx, RSP_ERR_NOMEM, "%s: host allocation failed", fn);
    } catch (const std::exception& e) {
        rc = fail(ctx, RSP_ERR_NOMEM, "%s: host pipeline: %s", fn, e.what());
    } catch (...) {
        rc = fail(ctx, RSP_ERR_NOMEM, "%s: host pipeline: unknown exception", fn);
    }
    if (rc && ctx->hp.s_h2d) {
        (void)hipStreamSynchronize(ctx->hp.s_h2d);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(ctx->hp.s_d2h);
    }
    return rc;
}

// Dev-only host-path trace (environment RSP_HOST_TRACE=1): per call, host time of the setup, the
// input staging (narrowing + DMA issue), the chain enqueue, the output staging (waits + widening)
// and the final syncs, plus device time of the H2D / chain / D2H streams (timing events), on
// stderr.  Used by tools/mex_bench.py --trace to find where a one-CPI MEX call spends its time.
struct HostTrace {
    const bool on;
    std::chrono::steady_clock::time_point t[8];
    int n = 0;
    hipEvent_t e[6] = {};
    double acc[3] = {};   // one-chunk path: input conversion, output waits, output conversion (us)
    explicit HostTrace(bool enable) : on(enable) {
        if (on)
            for (auto& x : e) (void)hipEventCreate(&x);
    }
    ~HostTrace() {
        if (on)
            for (auto& x : e) (void)hipEventDestroy(x);
    }
    HostTrace(const HostTrace&) = delete;
    void mark() { if (on && n < 8) t[n++] = std::chrono::steady_clock::now(); }
    double now_us() const {
        return on ? std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count() : 0.0;
    }
    void ev(int i, hipStream_t st) { if (on) (void)hipEventRecord(e[i], st); }
    // the call's line, after marks 0..5 and the streams' syncs; zc: the one-chunk form (no H2D stream)
    void report(int64_t batch, int64_t chunks, bool zc) const {
        if (!on) return;
        float g[3] = {};
        for (int i = zc ? 1 : 0; i < 3; ++i) (void)hipEventElapsedTime(&g[i], e[2 * i], e[2 * i + 1]);
        auto us = [&](int a, int b) { return std::chrono::duration<double, std::micro>(t[b] - t[a]).count(); };
        char h2d[32] = "0", tail[96] = "";
        if (zc) snprintf(tail, sizeof(tail), " zc_us narrow %.1f wait %.1f widen %.1f", acc[0], acc[1], acc[2]);
        else snprintf(h2d, sizeof(h2d), "%.1f", g[0] * 1e3);
        fprintf(stderr, "rsp_host_trace batch %lld chunks %lld%s host_us setup %.1f stage_in %.1f enqueue %.1f "
                "stage_out %.1f sync %.1f total %.1f dev_us h2d %s chain %.1f d2h %.1f%s\n", (long long)batch,
                (long long)chunks, zc ? " zc" : "", us(0, 1), us(1, 2), us(2, 3), us(3, 4), us(4, 5), us(0, 5), h2d,
                g[1] * 1e3, g[2] * 1e3, tail);
    }
};

// One-chunk calls (MATLAB's granularity: fun_MTD_produce is one CPI per call) are latency-bound,
// not bandwidth-bound: a pinned DMA pays ~13 us of fixed cost per copy and ~11 us more to
// signal the host (tools/micro/host_latency_probe.hip, profiles/r05/mex/), and the host's
// narrowing / widening sat between DMAs on the critical path.  Here the kernels move the data
// across PCIe themselves:
//   * input: the copy threads narrow (or copy) the caller's echo into pinned staging in pieces
//     of ~1 MiB that never cross a plane; right behind each piece, a transpose (column-major) or
//     copy (row-major) kernel on the chain's stream reads it from pinned memory into the
//     chain's device input -- PCIe transfer, ingest transpose and host narrowing overlap;
//   * output: after the chain, transpose / copy kernels write the RDM and flag planes into
//     pinned staging in up to kParts parts, an event behind each; the copy threads widen (or
//     copy) part q into the caller's arrays while parts q+1.. cross the link.
// Staging is allocated coherent (fine-grained: not cached in the GPU's L2), so a kernel never
// reads a previous call's input from L2 and the host never reads output lines the L2 still holds.
// RSP_HOST_ZC=0 (dev A/B) restores the DMA pipeline for every call.
static int zc_ensure(rsp_ctx* ctx, void** p, size_t* n, size_t bytes) {
    if (*p && *n >= bytes) return RSP_OK;
    if (*p) {
        HIP_TRY(ctx, hipHostFree(*p));
        *p = nullptr;
        *n = 0;
    }
    HIP_TRY(ctx, hipHostMalloc(p, bytes, knobs().zc == 2 ? hipHostMallocDefault : hipHostMallocCoherent));
    *n = bytes;
    return RSP_OK;
}

// device bytes per element a sub-block transpose reads (RSP_SUB_*; C32F16 writes complex float)
static size_t sub_size(int elem) { return elem == rsp::RSP_SUB_C64 ? 8 : (elem == rsp::RSP_SUB_U8 ? 1 : 4); }

// Input staging of the one-chunk paths: `planes` planes of the caller's `src`, converted piece
// by piece into the pinned staging (ctx->hp.zc_in, sized by the caller) with a release fence
// behind each piece, and right behind it a kernel on ctx->stream that reads the piece into
// `dst`: transposed (tr: a plane is the caller's [rows][cols], dst's [cols][rows]) or as it is.
static int zc_stage_in(rsp_ctx* ctx, const void* src, Conv conv, int elem, int64_t planes, int64_t rows, int64_t cols,
                       bool tr, void* dst, HostTrace& ht) {
    rsp::CopyPool& pool = host_pool(ctx);
    hipStream_t st = ctx->stream;
    char* zin = (char*)ctx->hp.zc_in;
    const size_t es = sub_size(elem), eout = elem == rsp::RSP_SUB_C32F16 ? 8 : es;
    auto stage = [&](size_t e0, size_t n) {   // elements [e0, e0 + n)
        const double t0 = ht.now_us();
        convert(pool, conv, zin + e0 * es, (const char*)src + rsp::conv_host_bytes(conv, e0 * es), n * es);
        std::atomic_thread_fence(std::memory_order_release);
        ht.acc[0] += ht.now_us() - t0;
    };
    if (tr) {
        for (const rsp::RowPiece& p : rsp::zc_in_rows(planes, rows, cols, es, knobs().piece)) {
            const size_t e0 = (size_t)(p.plane * rows + p.r0) * cols;
            stage(e0, (size_t)p.rows * cols);
            HIP_TRY(ctx, rsp::launch_transpose_sub(elem, zin + e0 * es,
                                                   (char*)dst + ((size_t)p.plane * rows * cols + p.r0) * eout,
                                                   (int)p.rows, (int)cols, (size_t)cols, (size_t)rows, st));
        }
    } else {
        for (const rsp::Span& s : rsp::zc_in_spans((size_t)planes * rows * cols, es, knobs().piece)) {
            stage(s.off, s.n);
            HIP_TRY(ctx, rsp::launch_copy_words(zin + s.off * es, (char*)dst + s.off * es, s.n * es / 4, st));
        }
    }
    return RSP_OK;
}

// Output delivery of the one-chunk paths: planes [batch][V][Ro] of each output (device, `es`
// bytes per element: 4 float, 1 byte) are transposed (tr: the caller's column-major [Ro][V]) or
// copied into pinned staging by kernels on ctx->stream, in parts of whole range-bin rows with an
// event behind each; the copy threads deliver part q -- converted by `conv` -- into the
// caller's array while the later parts cross the link.
struct ZcOut {
    const DevBuf* dev;   // (chain calls: slot 0's buffer of kSlots)
    size_t es;
    void* host;
    Conv conv;
};
static int zc_deliver(rsp_ctx* ctx, const ZcOut* outs, int nout, int64_t batch, int64_t V, int64_t Ro, bool tr,
                      HostTrace& ht) {
    auto& h = ctx->hp;
    const size_t cells = (size_t)V * Ro, ocells = (size_t)batch * cells;
    size_t es[3] = {}, zoff[4] = {};   // output k's staging is [zoff[k], zoff[k + 1])
    for (int k = 0; k < nout; ++k) {
        es[k] = outs[k].es;
        zoff[k + 1] = zoff[k] + ocells * es[k];
    }
    int rc;
    if ((rc = zc_ensure(ctx, &h.zc_out, &h.zc_out_n, zoff[nout]))) return rc;
    char* const zk[3] = {(char*)h.zc_out + zoff[0], (char*)h.zc_out + zoff[1], (char*)h.zc_out + zoff[2]};
    const std::vector<rsp::OutPart> parts = rsp::zc_out_parts(es, nout, batch, V, Ro, tr, knobs().part);
    if (parts.size() > (size_t)h.kParts) return fail(ctx, RSP_ERR_ARG, "one-chunk output: %zu parts", parts.size());
    hipStream_t st = ctx->stream;
    int np = 0;
    for (const rsp::OutPart& p : parts) {
        const char* d = (const char*)outs[p.k].dev->p;
        if (tr)   // plane b: [V][Ro] -> [Ro][V]; the part = output rows [c0, c0 + cols) (range bins)
            HIP_TRY(ctx, rsp::launch_transpose_sub(es[p.k] == 4 ? rsp::RSP_SUB_F32 : rsp::RSP_SUB_U8,
                                                   d + ((size_t)p.b * cells + p.c0) * es[p.k], zk[p.k] + p.off * es[p.k],
                                                   (int)V, (int)p.cols, (size_t)Ro, (size_t)V, st));
        else      // contiguous (whole 4-byte words: ocells % 4 == 0, zc_eligible)
            HIP_TRY(ctx, rsp::launch_copy_words(d + p.off * es[p.k], zk[p.k] + p.off * es[p.k], p.n * es[p.k] / 4, st));
        HIP_TRY(ctx, hipEventRecord(h.ev_part[np++], st));
    }
    ht.mark();   // 3: chain and output kernels enqueued
    rsp::CopyPool& pool = host_pool(ctx);
    for (int q = 0; q < np; ++q) {
        const rsp::OutPart& p = parts[(size_t)q];
        const ZcOut& o = outs[p.k];
        const double t0 = ht.now_us();
        HIP_TRY(ctx, hipEventSynchronize(h.ev_part[q]));
        const double t1 = ht.now_us();
        char* hp = (char*)o.host + rsp::conv_host_bytes(o.conv, p.off * o.es);
        if (h.pf) h.pf->wait(hp, rsp::conv_host_bytes(o.conv, p.n * o.es));
        convert(pool, o.conv, hp, zk[p.k] + p.off * o.es, p.n * o.es);
        ht.acc[1] += t1 - t0;
        ht.acc[2] += ht.now_us() - t1;
    }
    return RSP_OK;
}

// The one-chunk route of a chain call; taken = false (and nothing done): the DMA pipeline runs it.
// in / ddtype: the input's narrowing and what lands on the device; conv / tr: column-major input
// (transposed on the device) / outputs.
static int host_chain_small(rsp_ctx* ctx, const void* echo, Conv in, int32_t ddtype, bool conv, bool tr, int64_t P,
                            int64_t R, int64_t batch, const rsp_cfar_params* cfar, const ZcOut* outs, int no,
                            HostTrace& ht, bool& taken) {
    auto& h = ctx->hp;
    const int64_t Ro = ctx->p.R_out, V = ctx->V, planes = batch * ctx->beams;
    const size_t elems = (size_t)planes * P * R, dbytes = elems * dtype_size(ddtype);
    const size_t ocells = (size_t)batch * V * Ro;
    const bool want_fv = outs[no - 1].dev == h.flagV;
    taken = rsp::zc_eligible(dbytes, no, batch, ocells, conv, tr);
    if (!taken) return RSP_OK;
    int rc;
    if ((rc = zc_ensure(ctx, &h.zc_in, &h.zc_in_n, dbytes))) return rc;
    if ((rc = ensure(ctx, h.in[0], dbytes))) return rc;
    if (conv && (rc = ensure(ctx, h.canon[0], elems * sizeof(float2)))) return rc;
    if ((rc = ensure(ctx, h.rdm[0], ocells * sizeof(float)))) return rc;
    if (cfar && (rc = ensure(ctx, h.flag[0], ocells))) return rc;
    if (want_fv && (rc = ensure(ctx, h.flagV[0], ocells))) return rc;
    hipStream_t st = ctx->stream;
    // column-major: plane k = [R][P] -> canon [P][R]; row-major: copied as it is
    void* d_echo = conv ? h.canon[0].p : h.in[0].p;
    const int elem = ddtype == RSP_C32F16 ? rsp::RSP_SUB_C32F16 : rsp::RSP_SUB_C64;
    if ((rc = zc_stage_in(ctx, echo, in, elem, planes, R, P, conv, d_echo, ht))) return rc;
    ht.mark();   // 2: input staged
    ht.ev(2, st);
    rc = rsp_pc_mtd_cfar_dev(ctx, d_echo, conv ? RSP_C64 : ddtype, batch, cfar, (float*)h.rdm[0].p,
                             cfar ? (uint8_t*)h.flag[0].p : nullptr, want_fv ? (uint8_t*)h.flagV[0].p : nullptr, st);
    if (rc) return rc;
    ht.ev(3, st);
    ht.ev(4, st);
    if ((rc = zc_deliver(ctx, outs, no, batch, V, Ro, tr, ht))) return rc;
    ht.ev(5, st);
    ht.mark();   // 4: outputs delivered
    return RSP_OK;
}

// Prefault of the caller's output arrays (rsp_hostpool.h Prefaulter) from the start of a call
// whose outputs total >= kPrefaultMin bytes: new arrays of that size are fresh anonymous
// mappings (glibc serves allocations above its mmap threshold, at most 32 MiB, by mmap), and
// the copy threads would otherwise take one page fault + zeroing per 4 KiB as they deliver.
// The job ends (workers off the caller's memory) before the call returns, on every path.
// Dev A/B: RSP_PREFAULT=0 off; RSP_PREFAULT_THREADS (default 4); RSP_PREFAULT_HUGE=0 (no
// MADV_HUGEPAGE advice).  (Faulting on the calling thread's NUMA node was measured neutral on the
// GPU box -- every page landed on node 0 either way, profiles/r06/host/numa_ab/ -- and is not
// kept.)
struct PrefaultJob {
    rsp_ctx* ctx = nullptr;
    void begin(rsp_ctx* c, const std::vector<std::pair<void*, size_t>>& ranges) {
        const HostKnobs& kn = knobs();
        size_t total = 0;
        for (const auto& r : ranges) total += r.second;
        if (kn.prefault == 0 || total < rsp::kPrefaultMin) return;
        auto& h = c->hp;
        if (!h.prefault) h.prefault.reset(new rsp::Prefaulter(kn.prefault_threads, kn.prefault_huge != 0));
        h.prefault->begin(ranges);
        h.pf = h.prefault.get();
        ctx = c;
    }
    ~PrefaultJob() {
        if (ctx && ctx->hp.pf) {
            ctx->hp.pf->end();
            ctx->hp.pf = nullptr;
        }
    }
};

// The host-buffer chain: float / byte outputs, or (f64) MATLAB's double outputs.
static int host_chain(rsp_ctx* ctx, const void* echo, int32_t dtype, int32_t layout, int64_t P, int64_t R,
                      int64_t batch, const rsp_cfar_params* cfar, void* rdm_out, int32_t out_layout,
                      void* flag_out, void* flagV_out, bool f64) {
    HostTrace ht(knobs().trace);
    ht.mark();
    int rc = check_host_call(ctx, echo, dtype, layout, P, R, batch);
    if (rc) return rc;
    if (out_layout != RSP_ROWMAJOR && out_layout != RSP_COLMAJOR) return fail(ctx, RSP_ERR_ARG, "bad out_layout");
    if (cfar && !flag_out) return fail(ctx, RSP_ERR_ARG, "CFAR requested without flag_out");
    if (!cfar && !rdm_out) return fail(ctx, RSP_ERR_ARG, "no output requested");
    if (batch == 0) return RSP_OK;
    if ((rc = host_pipe_init(ctx))) return rc;
    auto& h = ctx->hp;
    const int64_t Ro = ctx->p.R_out, V = ctx->V, beams = ctx->beams;
    // MATLAB's complex double is narrowed to complex float by the host copy threads (the same
    // round-to-nearest cast the device conversion does): half the PCIe bytes
    const Conv in = dtype == RSP_C128 ? Conv::kC128toC64 : Conv::kNone;
    const int32_t ddtype = dtype == RSP_C128 ? RSP_C64 : dtype;              // what lands on the device
    const size_t in_cpi = (size_t)beams * P * R * dtype_size(dtype);         // caller's bytes
    const size_t dev_cpi = (size_t)beams * P * R * dtype_size(ddtype);       // device bytes
    const size_t cells = (size_t)V * Ro;   // per CPI
    const bool conv = layout != RSP_ROWMAJOR;   // column-major: transposed on the device
    const bool tr = out_layout == RSP_COLMAJOR;
    const bool want_fv = cfar && flagV_out;
    ZcOut outs[3];   // the outputs asked for; output q of slot sl: outs[q].dev[sl], transposed in h.tr[sl][q]
    int no = 0;
    if (rdm_out) outs[no++] = {h.rdm, 4, rdm_out, f64 ? Conv::kF32toF64 : Conv::kNone};
    if (cfar) outs[no++] = {h.flag, 1, flag_out, f64 ? Conv::kU8toF64 : Conv::kNone};
    if (want_fv) outs[no++] = {h.flagV, 1, flagV_out, f64 ? Conv::kU8toF64 : Conv::kNone};
    auto host_bytes = [&](const ZcOut& o, size_t ncells) { return rsp::conv_host_bytes(o.conv, ncells * o.es); };
    const rsp::HostChunks ch = rsp::host_chunks(batch, ctx->host_chunk, dev_cpi);
    const int64_t K = ch.K, nk = ch.nk;
    PrefaultJob pfjob;   // (ends the prefault job on every return below)
    std::vector<std::pair<void*, size_t>> fresh;
    for (int q = 0; q < no; ++q) fresh.push_back({outs[q].host, host_bytes(outs[q], (size_t)batch * cells)});
    pfjob.begin(ctx, fresh);
    if (nk == 1 && knobs().zc != 0) {
        ht.mark();   // 1: set up
        bool taken = false;
        rc = host_chain_small(ctx, echo, in, ddtype, conv, tr, P, R, batch, cfar, outs, no, ht, taken);
        if (taken) {
            if (rc == RSP_OK && ht.on) {
                ht.mark();   // 5
                (void)hipStreamSynchronize(ctx->stream);
                ht.report(batch, 1, true);
            }
            return rc;
        }
        ht.n = 1;   // (the DMA pipeline's marks follow)
    }
    for (int i = 0; i < h.kSlots && i < nk; ++i) {
        if ((rc = ensure(ctx, h.in[i], (size_t)K * dev_cpi))) return rc;
        if (conv && (rc = ensure(ctx, h.canon[i], (size_t)K * beams * P * R * sizeof(float2)))) return rc;
        if ((rc = ensure(ctx, h.rdm[i], (size_t)K * cells * sizeof(float)))) return rc;
        if (cfar && (rc = ensure(ctx, h.flag[i], (size_t)K * cells))) return rc;
        if (want_fv && (rc = ensure(ctx, h.flagV[i], (size_t)K * cells))) return rc;
        for (int q = 0; tr && q < no; ++q)
            if ((rc = ensure(ctx, h.tr[i][q], (size_t)K * cells * outs[q].es))) return rc;
    }
    // chunk k: the chain on slot k % 2 after its H2D, then transposes; its outputs' D2H waits for it
    auto compute = [&](int64_t k) -> int {
        const int sl = (int)(k % h.kSlots);
        const int64_t n = ch.size(k);
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, h.ev_in[sl], 0));
        if (k >= h.kSlots) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, h.ev_out[sl], 0));   // slot's D2H done
        const void* d_echo = h.in[sl].p;
        int32_t d_dtype = ddtype;
        if (conv) {
            HIP_TRY(ctx, rsp::launch_canon(h.in[sl].p, ddtype, layout, (float2*)h.canon[sl].p, n * beams, (int)P,
                                           (int)R, ctx->stream));
            d_echo = h.canon[sl].p;
            d_dtype = RSP_C64;
        }
        int rc2 = rsp_pc_mtd_cfar_dev(ctx, d_echo, d_dtype, n, cfar, (float*)h.rdm[sl].p,
                                      cfar ? (uint8_t*)h.flag[sl].p : nullptr,
                                      want_fv ? (uint8_t*)h.flagV[sl].p : nullptr, ctx->stream);
        if (rc2) return rc2;
        for (int q = 0; tr && q < no; ++q) {
            const void* d = outs[q].dev[sl].p;
            void* t = h.tr[sl][q].p;
            HIP_TRY(ctx, outs[q].es == 4
                             ? rsp::launch_transpose_f32((const float*)d, (float*)t, n, (int)V, (int)Ro, ctx->stream)
                             : rsp::launch_transpose_u8((const uint8_t*)d, (uint8_t*)t, n, (int)V, (int)Ro, ctx->stream));
        }
        HIP_TRY(ctx, hipEventRecord(h.ev_comp[sl], ctx->stream));
        return RSP_OK;
    };
    auto output = [&](int64_t k) -> int {
        const int sl = (int)(k % h.kSlots);
        const size_t n = (size_t)ch.size(k), o = (size_t)k * K * cells;
        HIP_TRY(ctx, hipStreamWaitEvent(h.s_d2h, h.ev_comp[sl], 0));
        std::vector<D2HPart> parts;
        for (int q = 0; q < no; ++q)
            parts.push_back({tr ? h.tr[sl][q].p : outs[q].dev[sl].p,
                             (char*)outs[q].host + host_bytes(outs[q], o), n * cells * outs[q].es, outs[q].conv});
        int rc2 = d2h_pieces(ctx, parts);
        if (rc2) return rc2;
        HIP_TRY(ctx, hipEventRecord(h.ev_out[sl], h.s_d2h));
        return RSP_OK;
    };
    ht.mark();   // 1: set up
    for (int64_t k = 0; k < nk; ++k) {
        const int sl = (int)(k % h.kSlots);
        // the slot's previous chain (chunk k-2) has read its input
        if (k >= h.kSlots) HIP_TRY(ctx, hipStreamWaitEvent(h.s_h2d, h.ev_comp[sl], 0));
        if (k == 0) ht.ev(0, h.s_h2d);
        if ((rc = h2d_pieces(ctx, h.in[sl].p, (const char*)echo + (size_t)k * K * in_cpi, (size_t)ch.size(k) * dev_cpi, in)))
            return rc;
        if (k == nk - 1) ht.ev(1, h.s_h2d);
        HIP_TRY(ctx, hipEventRecord(h.ev_in[sl], h.s_h2d));
        if (k == 0) ht.mark();   // 2: first chunk staged
        if (k == 0) {
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, h.ev_in[sl], 0));
            ht.ev(2, ctx->stream);
        }
        if ((rc = compute(k))) return rc;
        if (k == nk - 1) ht.ev(3, ctx->stream);
        if (k == 0) ht.mark();   // 3: first chain enqueued
        if (k >= 1 && (rc = output(k - 1))) return rc;
    }
    if (ht.on) {
        HIP_TRY(ctx, hipStreamWaitEvent(h.s_d2h, h.ev_comp[(nk - 1) % h.kSlots], 0));
        ht.ev(4, h.s_d2h);
    }
    if ((rc = output(nk - 1))) return rc;
    ht.ev(5, h.s_d2h);
    ht.mark();   // 4: outputs staged
    HIP_TRY(ctx, hipStreamSynchronize(h.s_d2h));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ht.mark();   // 5: done
    ht.report(batch, nk, false);
    return RSP_OK;
}

static int host_call(rsp_ctx* ctx, const void* echo, int32_t dtype, int32_t layout, int64_t P, int64_t R,
                     int64_t batch, const rsp_cfar_params* cfar, void* rdm_out, int32_t out_layout, void* flag_out,
                     void* flagV_out, bool f64) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "null ctx");
    return drained(ctx, "rsp_pc_mtd_cfar", [&] {
        return host_chain(ctx, echo, dtype, layout, P, R, batch, cfar, rdm_out, out_layout, flag_out, flagV_out, f64);
    });
}

int rsp_pc_mtd_cfar(rsp_ctx* ctx, const void* echo, int32_t dtype, int32_t layout, int64_t P, int64_t R,
                    int64_t batch, const rsp_cfar_params* cfar, float* rdm_out, int32_t out_layout,
                    uint8_t* flag_out, uint8_t* flagV_out) {
    return host_call(ctx, echo, dtype, layout, P, R, batch, cfar, rdm_out, out_layout, flag_out, flagV_out, false);
}

int rsp_pc_mtd_cfar_f64(rsp_ctx* ctx, const void* echo, int32_t dtype, int32_t layout, int64_t P, int64_t R,
                        int64_t batch, const rsp_cfar_params* cfar, double* rdm_out, int32_t out_layout,
                        double* flag_out, double* flagV_out) {
    return host_call(ctx, echo, dtype, layout, P, R, batch, cfar, rdm_out, out_layout, flag_out, flagV_out, true);
}

int rsp_pc_mtd(rsp_ctx* ctx, const void* echo, int32_t dtype, int32_t layout, int64_t P, int64_t R,
               int64_t batch, float* rdm_out, int32_t rdm_layout) {
    if (!rdm_out) return fail(ctx, RSP_ERR_ARG, "rsp_pc_mtd: null rdm_out");
    return rsp_pc_mtd_cfar(ctx, echo, dtype, layout, P, R, batch, nullptr, rdm_out, rdm_layout, nullptr, nullptr);
}

int rsp_cfar(rsp_ctx* ctx, const float* rdm, int32_t rdm_layout, int64_t V, int64_t R, int64_t batch,
             const rsp_cfar_params* cfar, uint8_t* flag_out, uint8_t* flagV_out) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "null ctx");
    if (!rdm || !cfar || !flag_out || V < 1 || R < 1 || batch < 0) return fail(ctx, RSP_ERR_ARG, "rsp_cfar: bad argument");
    if (rdm_layout != RSP_ROWMAJOR && rdm_layout != RSP_COLMAJOR) return fail(ctx, RSP_ERR_ARG, "bad rdm_layout");
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    const size_t cells = (size_t)batch * V * R;
    int rc;
    if ((rc = ensure(ctx, ctx->st_in, cells * sizeof(float)))) return rc;
    if ((rc = ensure(ctx, ctx->st_rdm, cells * sizeof(float)))) return rc;
    if ((rc = ensure(ctx, ctx->st_flag, cells))) return rc;
    if ((rc = ensure(ctx, ctx->st_flagV, cells))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->st_in.p, rdm, cells * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    const float* d_rdm = (const float*)ctx->st_in.p;
    if (rdm_layout == RSP_COLMAJOR) {  // MATLAB V x R = [b][R][V] -> [b][V][R]
        HIP_TRY(ctx, rsp::launch_transpose_f32(d_rdm, (float*)ctx->st_rdm.p, batch, (int)R, (int)V, ctx->stream));
        d_rdm = (const float*)ctx->st_rdm.p;
    }
    rc = rsp_cfar_dev(ctx, d_rdm, V, R, batch, cfar, (uint8_t*)ctx->st_flag.p, (uint8_t*)ctx->st_flagV.p, ctx->stream);
    if (rc) return rc;
    if ((rc = fetch(ctx, (const uint8_t*)ctx->st_flag.p, flag_out, batch, V, R, rdm_layout))) return rc;
    if (flagV_out && (rc = fetch(ctx, (const uint8_t*)ctx->st_flagV.p, flagV_out, batch, V, R, rdm_layout)))
        return rc;
    return RSP_OK;
}

// executeCFAR with MATLAB's types (rsp.h): the double RDM narrowed to float by the copy pool on
// its way into pinned memory, the 0/1 flags widened to double as their parts or pieces land.
static int cfar_f64_body(rsp_ctx* ctx, const double* rdm, int32_t rdm_layout, int64_t V, int64_t R, int64_t batch,
                         const rsp_cfar_params* cfar, double* flag_out, double* flagV_out) {
    int rc;
    if ((rc = host_pipe_init(ctx))) return rc;
    const size_t cells = (size_t)batch * V * R;
    if ((rc = ensure(ctx, ctx->st_in, cells * sizeof(float)))) return rc;
    if ((rc = ensure(ctx, ctx->st_rdm, cells * sizeof(float)))) return rc;
    if ((rc = ensure(ctx, ctx->st_flag, cells))) return rc;
    if ((rc = ensure(ctx, ctx->st_flagV, cells))) return rc;
    auto& h = ctx->hp;
    const bool col = rdm_layout == RSP_COLMAJOR;
    const int nout = flagV_out ? 2 : 1;
    if (knobs().zc != 0 && rsp::zc_eligible(cells * sizeof(float), nout, batch, cells, col, col)) {
        // one chunk (executeCFAR's segments); column-major: plane k = [R][V] -> [V][R]
        if ((rc = zc_ensure(ctx, &h.zc_in, &h.zc_in_n, cells * sizeof(float)))) return rc;
        HostTrace none(false);
        if ((rc = zc_stage_in(ctx, rdm, Conv::kF64toF32, rsp::RSP_SUB_F32, batch, R, V, col,
                              col ? ctx->st_rdm.p : ctx->st_in.p, none)))
            return rc;
        rc = rsp_cfar_dev(ctx, (const float*)(col ? ctx->st_rdm.p : ctx->st_in.p), V, R, batch, cfar,
                          (uint8_t*)ctx->st_flag.p, (uint8_t*)ctx->st_flagV.p, ctx->stream);
        if (rc) return rc;
        ZcOut outs[2] = {{&ctx->st_flag, 1, flag_out, Conv::kU8toF64}, {&ctx->st_flagV, 1, flagV_out, Conv::kU8toF64}};
        return zc_deliver(ctx, outs, nout, batch, V, R, col, none);
    }
    if ((rc = h2d_pieces(ctx, ctx->st_in.p, rdm, cells * sizeof(float), Conv::kF64toF32))) return rc;
    HIP_TRY(ctx, hipEventRecord(h.ev_in[0], h.s_h2d));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, h.ev_in[0], 0));
    const float* d_rdm = (const float*)ctx->st_in.p;
    if (col) {  // MATLAB V x R = [b][R][V] -> [b][V][R]
        HIP_TRY(ctx, rsp::launch_transpose_f32(d_rdm, (float*)ctx->st_rdm.p, batch, (int)R, (int)V, ctx->stream));
        d_rdm = (const float*)ctx->st_rdm.p;
    }
    rc = rsp_cfar_dev(ctx, d_rdm, V, R, batch, cfar, (uint8_t*)ctx->st_flag.p, (uint8_t*)ctx->st_flagV.p, ctx->stream);
    if (rc) return rc;
    const uint8_t* f = (const uint8_t*)ctx->st_flag.p;
    const uint8_t* fv = (const uint8_t*)ctx->st_flagV.p;
    if (col) {   // back to MATLAB's [b][R][V]
        if ((rc = ensure(ctx, ctx->st_t, cells))) return rc;
        if ((rc = ensure(ctx, ctx->st_canon, cells))) return rc;
        HIP_TRY(ctx, rsp::launch_transpose_u8(f, (uint8_t*)ctx->st_t.p, batch, (int)V, (int)R, ctx->stream));
        f = (const uint8_t*)ctx->st_t.p;
        if (flagV_out) {
            HIP_TRY(ctx, rsp::launch_transpose_u8(fv, (uint8_t*)ctx->st_canon.p, batch, (int)V, (int)R, ctx->stream));
            fv = (const uint8_t*)ctx->st_canon.p;
        }
    }
    HIP_TRY(ctx, hipEventRecord(h.ev_comp[0], ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(h.s_d2h, h.ev_comp[0], 0));
    std::vector<D2HPart> parts;
    parts.push_back({f, flag_out, cells, Conv::kU8toF64});
    if (flagV_out) parts.push_back({fv, flagV_out, cells, Conv::kU8toF64});
    if ((rc = d2h_pieces(ctx, parts))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(h.s_d2h));
    return RSP_OK;
}

int rsp_cfar_f64(rsp_ctx* ctx, const double* rdm, int32_t rdm_layout, int64_t V, int64_t R, int64_t batch,
                 const rsp_cfar_params* cfar, double* flag_out, double* flagV_out) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "null ctx");
    if (!rdm || !cfar || !flag_out || V < 1 || R < 1 || batch < 0) return fail(ctx, RSP_ERR_ARG, "rsp_cfar_f64: bad argument");
    if (rdm_layout != RSP_ROWMAJOR && rdm_layout != RSP_COLMAJOR) return fail(ctx, RSP_ERR_ARG, "bad rdm_layout");
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    return drained(ctx, "rsp_cfar_f64", [&] { return cfar_f64_body(ctx, rdm, rdm_layout, V, R, batch, cfar, flag_out, flagV_out); });
}
