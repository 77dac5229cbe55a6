// rsp_capi.cpp -- the C ABI (include/rsp.h): context, parameter validation, fp64 host
// precomputation (matched-filter spectra, twiddle tables, windows), device buffer pools
// and the chunked PC -> MTD(+Doppler CFAR) -> range CFAR pipeline.  The entry points of the
// stages around the chain are in rsp_stages.cpp, the host-buffer ones in rsp_host.cpp.
//
// Chunking: the pulse-compression output of `chunk` CPIs is written to a scratch buffer
// that is read back by the MTD kernel right after; chunk * P * R_out * 8 bytes is sized
// (default 64 MiB) to stay in the 256 MiB Infinity Cache, so the corner turn between
// the fast-time (PC) and slow-time (MTD) passes is served on-die instead of from HBM.
#include <hip/hip_runtime.h>

#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "rsp_ctx.h"
#include "rsp_pcplan.h"

using rsp::make_window;
using rsp::scratch_acquire;
using rsp::scratch_release;
using rsp::upload;

using cd = std::complex<double>;

static thread_local std::string g_err;

int fail(rsp_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    g_err = buf;
    return code;
}


// ------------------------------------------------------------------ host numerics (fp64)
static double mround(double x) { return x >= 0 ? std::floor(x + 0.5) : -std::floor(-x + 0.5); }

static double bessel_i0(double x) {
    double sum = 1.0, term = 1.0, q = x * x / 4.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

std::vector<double> rsp::make_window(int kind, double beta, int64_t n) {
    std::vector<double> w((size_t)n, 1.0);
    if (n == 1) return w;
    for (int64_t k = 0; k < n; ++k) {
        if (kind == RSP_WIN_KAISER) {
            double r = ((double)k - (n - 1) / 2.0) / ((n - 1) / 2.0);
            double a = 1.0 - r * r;
            w[k] = bessel_i0(beta * std::sqrt(a > 0 ? a : 0.0)) / bessel_i0(beta);
        } else if (kind == RSP_WIN_HAMMING) {
            w[k] = 0.54 - 0.46 * std::cos(2.0 * M_PI * (double)k / (double)(n - 1));
        }
    }
    return w;
}

// in-place radix-2 forward FFT, n a power of two
static void fft_pow2(std::vector<cd>& a) {
    const size_t n = a.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        for (size_t i = 0; i < n; i += len) {
            for (size_t k = 0; k < len / 2; ++k) {
                const double ang = -2.0 * M_PI * (double)k / (double)len;
                const cd w(std::cos(ang), std::sin(ang));
                const cd u = a[i + k], v = a[i + k + len / 2] * w;
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
            }
        }
    }
}

static int twiddles(rsp_ctx* ctx, int n, const float2** out) {
    auto it = ctx->tw.find(n);
    if (it != ctx->tw.end()) {
        *out = it->second;
        return RSP_OK;
    }
    std::vector<float2> h((size_t)n);
    for (int e = 0; e < n; ++e) {
        const double ang = -2.0 * M_PI * (double)e / (double)n;
        h[e] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
    float2* d = nullptr;
    int rc = upload(ctx, h, &d);
    if (rc) return rc;
    ctx->tw[n] = d;
    *out = d;
    return RSP_OK;
}

// H = conj(FFT_n(scale * replica)) / n in fp64 (fft(x, n) truncates), and the n-point twiddles
static int mf_spectrum(rsp_ctx* ctx, const rsp_pc_segment& g, int n, const float2** H, const float2** tw) {
    std::vector<cd> a((size_t)n, cd(0, 0));
    const int64_t L = g.coef_len < n ? g.coef_len : n;
    for (int64_t k = 0; k < L; ++k) a[k] = g.scale * cd(g.coef_re[k], g.coef_im ? g.coef_im[k] : 0.0);
    fft_pow2(a);
    std::vector<float2> h((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        const cd v = std::conj(a[k]) / (double)n;
        h[k] = make_float2((float)v.real(), (float)v.imag());
    }
    float2* dh = nullptr;
    int rc = upload(ctx, h, &dh);
    if (rc) return rc;
    *H = dh;
    return twiddles(ctx, n, tw);
}

// Overlap-save split of a long matched-filter segment (fun_lss_pulse_compression.m:64-72:
// ifft(fft(x, nfft) .* conj(fft(h, nfft)))).  With nfft >= out_len + hlen - 1 no output of the
// nfft-point circular correlation wraps, so output n = sum_k x[n + k] conj(h[k]) (x zero past
// in_len) -- the same sums as nsub blocks of an nb-point correlation, block j producing outputs
// [j*step, (j+1)*step), step = nb - hlen + 1.  A 16384-point row needs one 139 KB LDS slot
// (one workgroup per CU, every phase exposed); nb = 4096 blocks run four workgroups per CU.
// Kept only where it is exact in that sense and the FIR does not ride on the segment.
static int pc_overlap_save(rsp_ctx* ctx, const rsp_pc_segment& g, rsp::PcMfArgs& a) {
    a.nsub = 0;
    a.sub_step = 0;
    const int64_t nfft = a.mf.nfft;
    const int64_t hlen = g.coef_len < nfft ? g.coef_len : nfft;
    if (nfft <= ctx->pc_ols_min || a.do_fir || nfft < (int64_t)a.mf.out_len + hlen - 1) return RSP_OK;
    int best = 0, best_n = 0, best_step = 0;
    for (int nb : {8192, 4096, 2048}) {   // (ties: the longer block, fewer re-read samples)
        if (nb >= nfft) continue;
        const int64_t step = nb - hlen + 1;
        if (step < nb / 2) continue;
        const int64_t n = (a.mf.out_len + step - 1) / step;
        if (!best || n * nb < (int64_t)best_n * best) {
            best = nb;
            best_n = (int)n;
            best_step = (int)step;
        }
    }
    if (!best || (int64_t)best_n * best >= 2 * nfft) return RSP_OK;
    int rc = mf_spectrum(ctx, g, best, &a.mf.H, &a.mf.tw);
    if (rc) return rc;
    a.mf.nfft = best;
    a.nsub = best_n;
    a.sub_step = best_step;
    return RSP_OK;
}

// PcMfArgs::zin / zout of a segment (after the overlap-save decision): whole slices of
// G = nfft/16 points past the longest input / output window of any sub-block.
static void pc_prune_counts(rsp::PcMfArgs& a) {
    a.zin = a.zout = 0;
    const int n = a.mf.nfft, g = n / 16;
    if (g < 64 || g % 64) return;   // only wave-uniform rows range-check by buffer resource
    int in = a.mf.in_len, out = a.mf.out_len;
    if (a.nsub > 1) out = out < a.sub_step ? out : a.sub_step;   // (sub-block 0 has the longest windows)
    in = in < 0 ? 0 : in < n ? in : n;
    out = out < 0 ? 0 : out < n ? out : n;
    a.zin = (n - in) / g;
    a.zout = (n - out) / g;
}

int ensure(rsp_ctx* ctx, DevBuf& b, size_t bytes) {
    if (b.n >= bytes && b.p) return RSP_OK;
    if (b.p) {
        HIP_TRY(ctx, hipFree(b.p));
        b.p = nullptr;
        b.n = 0;
    }
    if (bytes == 0) return RSP_OK;
    HIP_TRY(ctx, hipMalloc(&b.p, bytes));
    b.n = bytes;
    return RSP_OK;
}

static void zero_v_band(int64_t rows, int div, int* lo, int* hi) {
    if (div <= 0) {
        *lo = 0;
        *hi = 0;
        return;
    }
    const int64_t zv = (int64_t)mround(rows / 2.0);
    const int64_t k = (int64_t)mround((double)rows / (double)div);
    int64_t a = zv - k - 1, b = zv + k;
    if (a < 0) a = 0;
    if (b > rows) b = rows;
    *lo = (int)a;
    *hi = (int)(b > a ? b : a);
}

// ------------------------------------------------------------------ public API
const char* rsp_version(void) { return "rsp-mi355x 0.5.0 (gfx950, abi 5)"; }

const char* rsp_last_error(const rsp_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int rsp_destroy(rsp_ctx* ctx) {
    if (!ctx) return RSP_OK;
    hipSetDevice(ctx->device);
    for (void* p : ctx->owned) hipFree(p);
    DevBuf* bufs[] = {&ctx->pf_gain, &ctx->scratch_pc, &ctx->cat_tmp, &ctx->tmp_flagV, &ctx->tmp_rdm, &ctx->hit_list, &ctx->hit_ctr,
                      &ctx->st_in, &ctx->st_canon, &ctx->st_rdm, &ctx->st_flag, &ctx->st_flagV, &ctx->st_t,
                      &ctx->meas_band, &ctx->ing_meta, &ctx->scr_ps, &ctx->cond_tmp, &ctx->cmap_band,
                      &ctx->integ_plan};
    for (DevBuf* b : bufs)
        if (b->p) hipFree(b->p);
    for (auto& e : ctx->evs) {
        hipEventDestroy(e.a);
        hipEventDestroy(e.b);
    }
    for (int i = 0; i < 3; ++i) {
        if (ctx->aux[i]) hipStreamDestroy(ctx->aux[i]);
        if (ctx->ev_join[i]) hipEventDestroy(ctx->ev_join[i]);
    }
    {
        auto& h = ctx->hp;
        for (int i = 0; i < h.kSlots; ++i) {
            DevBuf* hb[] = {&h.in[i], &h.canon[i], &h.rdm[i], &h.flag[i], &h.flagV[i], &h.tr[i][0], &h.tr[i][1],
                            &h.tr[i][2]};
            for (DevBuf* b : hb)
                if (b->p) hipFree(b->p);
            if (h.ev_in[i]) hipEventDestroy(h.ev_in[i]);
            if (h.ev_comp[i]) hipEventDestroy(h.ev_comp[i]);
            if (h.ev_out[i]) hipEventDestroy(h.ev_out[i]);
        }
        if (h.zc_in) hipHostFree(h.zc_in);
        if (h.zc_out) hipHostFree(h.zc_out);
        for (auto& e : h.ev_part)
            if (e) hipEventDestroy(e);
        for (int i = 0; i < h.kRing; ++i) {
            if (h.pin_in[i]) hipHostFree(h.pin_in[i]);
            if (h.pin_out[i]) hipHostFree(h.pin_out[i]);
            if (h.ev_pin_in[i]) hipEventDestroy(h.ev_pin_in[i]);
            if (h.ev_pin_out[i]) hipEventDestroy(h.ev_pin_out[i]);
        }
        if (h.s_h2d) hipStreamDestroy(h.s_h2d);
        if (h.s_d2h) hipStreamDestroy(h.s_d2h);
        h.pool.reset();
    }
    if (ctx->ev_fork) hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_scratch) hipEventDestroy(ctx->ev_scratch);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
    return RSP_OK;
}

int rsp_create(rsp_ctx** out, int device, const rsp_params* prm) {
    if (!out) return fail(nullptr, RSP_ERR_ARG, "rsp_create: null argument");
    *out = nullptr;
    if (!prm) {   // CFAR-only context (rsp_cfar / rsp_cfar_dev): a device and a stream
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            return fail(nullptr, RSP_ERR_HIP, "rsp_create: no HIP device available");
        if (device < 0 || device >= ndev)
            return fail(nullptr, RSP_ERR_ARG, "rsp_create: device %d out of range (%d devices)", device, ndev);
        rsp_ctx* ctx = new rsp_ctx();
        ctx->device = device;
        ctx->cfar_only = true;
        if (hipSetDevice(device) != hipSuccess ||
            hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
            delete ctx;
            return fail(nullptr, RSP_ERR_HIP, "rsp_create: device/stream setup failed");
        }
        *out = ctx;
        return RSP_OK;
    }
    const rsp_params& p = *prm;
    if (p.P < 2 || p.R < 1 || p.R_out < 1 || p.R > (1 << 24) || p.R_out > (1 << 24))
        return fail(nullptr, RSP_ERR_SHAPE, "rsp_create: bad P=%lld R=%lld R_out=%lld",
                    (long long)p.P, (long long)p.R, (long long)p.R_out);
    const int64_t V = p.mtd_nfft ? p.mtd_nfft : p.P;
    const int beams = p.beams ? p.beams : 1;
    if (beams < 1 || beams > 2) return fail(nullptr, RSP_ERR_ARG, "rsp_create: beams=%d (1 or 2)", p.beams);
    if (V < p.P)
        return fail(nullptr, RSP_ERR_SHAPE, "rsp_create: mtd_nfft=%lld < P=%lld", (long long)V, (long long)p.P);
    const bool bluestein = !rsp::mtd_size_supported((int)V, beams) && beams == 1 && V == p.P &&
                           rsp::mtd_bluestein_nf((int)V) > 0;
    if (!rsp::mtd_size_supported((int)V, beams) && !bluestein)
        return fail(nullptr, RSP_ERR_UNSUPPORTED,
                    "rsp_create: Doppler length %lld (beams %d) not built (radix plans 2^k, 3*2^k up to 2048; "
                    "other even and odd P <= 1024 by Bluestein; two beams: 512, 1024, 2048)",
                    (long long)V, beams);
    if (p.zero_ends < 0 || 2 * (int64_t)p.zero_ends > V)
        return fail(nullptr, RSP_ERR_ARG, "rsp_create: zero_ends=%d out of range", p.zero_ends);
    if (p.nseg < 0 || p.nseg > RSP_MAX_SEG)
        return fail(nullptr, RSP_ERR_ARG, "rsp_create: nseg=%d out of range", p.nseg);
    if (p.window < RSP_WIN_KAISER || p.window > RSP_WIN_RECT)
        return fail(nullptr, RSP_ERR_ARG, "rsp_create: bad window %d", p.window);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, RSP_ERR_HIP, "rsp_create: no HIP device available");
    if (device < 0 || device >= ndev)
        return fail(nullptr, RSP_ERR_ARG, "rsp_create: device %d out of range (%d devices)", device, ndev);

    rsp_ctx* ctx = new rsp_ctx();
    ctx->device = device;
    ctx->p = p;
    ctx->pc_w = p.R_out;
    for (int s = 0; s < RSP_MAX_SEG; ++s) ctx->p.seg[s].coef_re = ctx->p.seg[s].coef_im = nullptr;
    auto bail = [&](int rc) {
        g_err = ctx->err;
        rsp_destroy(ctx);
        return rc;
    };
    if (hipSetDevice(device) != hipSuccess) return bail(fail(ctx, RSP_ERR_HIP, "hipSetDevice(%d) failed", device));
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(ctx, RSP_ERR_HIP, "hipStreamCreate failed"));

    // ---- pulse-compression segments
    rsp::PcArgs& pc = ctx->pc;
    pc.P = (int)p.P;
    pc.R = (int)p.R;
    pc.R_out = (int)p.R_out;
    pc.nseg = p.nseg;
    std::vector<char> covered((size_t)p.R_out, 0);
    int max_nfft = 64;
    for (int s = 0; s < p.nseg; ++s) {
        const rsp_pc_segment& g = p.seg[s];
        rsp::SegDev& d = pc.seg[s];
        std::memset(&d, 0, sizeof(d));
        if (g.in_start < 0 || g.in_len < 1 || g.in_start + g.in_len > p.R)
            return bail(fail(ctx, RSP_ERR_ARG, "segment %d: input [%lld,+%lld) outside R=%lld", s,
                             (long long)g.in_start, (long long)g.in_len, (long long)p.R));
        if (g.out_start < 0 || g.out_len < 1 || g.out_start + g.out_len > p.R_out)
            return bail(fail(ctx, RSP_ERR_ARG, "segment %d: output [%lld,+%lld) outside R_out=%lld", s,
                             (long long)g.out_start, (long long)g.out_len, (long long)p.R_out));
        for (int64_t c = g.out_start; c < g.out_start + g.out_len; ++c) {
            if (covered[c]) return bail(fail(ctx, RSP_ERR_ARG, "segment %d overlaps another segment's output", s));
            covered[c] = 1;
        }
        if (!g.coef_re || g.coef_len < 1)
            return bail(fail(ctx, RSP_ERR_ARG, "segment %d: missing coefficients", s));
        d.kind = g.kind;
        d.in_start = (int)g.in_start;
        d.in_len = (int)g.in_len;
        d.out_start = (int)g.out_start;
        d.out_len = (int)g.out_len;
        d.scale = (float)g.scale;
        if (g.kind == RSP_SEG_FIR) {
            if (g.coef_len > RSP_MAX_FIR_TAPS)
                return bail(fail(ctx, RSP_ERR_UNSUPPORTED, "segment %d: %lld FIR taps > %d", s,
                                 (long long)g.coef_len, RSP_MAX_FIR_TAPS));
            if (g.out_len != g.in_len)
                return bail(fail(ctx, RSP_ERR_ARG, "segment %d: FIR needs out_len == in_len", s));
            d.ntaps = (int)g.coef_len;
            std::vector<float> tf((size_t)d.ntaps);
            for (int k = 0; k < d.ntaps; ++k) d.taps[k] = tf[k] = (float)g.coef_re[k];
            float* dt = nullptr;
            int rc = upload(ctx, tf, &dt);
            if (rc) return bail(rc);
            d.taps_dev = dt;
            d.ntaps4 = (d.ntaps + 3) & ~3;
            std::vector<float2> t2((size_t)d.ntaps4, float2{0.f, 0.f});
            for (int k = 0; k < d.ntaps; ++k) {
                const float b = (float)(g.coef_re[k] * g.scale);
                t2[k] = float2{b, b};
            }
            float2* dt2 = nullptr;
            rc = upload(ctx, t2, &dt2);
            if (rc) return bail(rc);
            d.taps2_dev = dt2;
            int64_t sh = g.fir_shift % g.out_len;
            if (sh < 0) sh += g.out_len;
            d.fir_shift = (int)sh;
        } else if (g.kind == RSP_SEG_MF) {
            if (!rsp::pc_nfft_supported((int)g.nfft))
                return bail(fail(ctx, RSP_ERR_UNSUPPORTED, "segment %d: nfft=%lld not built (2^k, 64..16384)", s,
                                 (long long)g.nfft));
            if (g.in_len > g.nfft || g.out_len > g.nfft)
                return bail(fail(ctx, RSP_ERR_ARG, "segment %d: in_len/out_len exceed nfft", s));
            d.nfft = (int)g.nfft;
            if (d.nfft > max_nfft) max_nfft = d.nfft;
            int rc = mf_spectrum(ctx, g, d.nfft, &d.H, &d.tw);
            if (rc) return bail(rc);
        } else {
            return bail(fail(ctx, RSP_ERR_ARG, "segment %d: bad kind %d", s, g.kind));
        }
    }
    // output columns no segment writes stay 0 (s_PC_0 = zeros, fun_lss_pulse_compression.m:27)
    pc.nzero = 0;
    for (int64_t c = 0; c < p.R_out;) {
        if (covered[c]) { ++c; continue; }
        int64_t e = c;
        while (e < p.R_out && !covered[e]) ++e;
        if (pc.nzero >= RSP_MAX_SEG + 1)
            return bail(fail(ctx, RSP_ERR_UNSUPPORTED, "too many uncovered output column ranges"));
        pc.zero_lo[pc.nzero] = (int)c;
        pc.zero_hi[pc.nzero] = (int)e;
        ++pc.nzero;
        c = e;
    }
    ctx->pc_lds = rsp::pc_lds_bytes(max_nfft);
    // Specialised path: at most one FIR segment, every MF length built, FIR staged in a slot
    {
        int nfir = 0, nmf = 0, fir_idx = -1;
        bool ok = true;
        for (int s = 0; s < p.nseg; ++s) {
            if (pc.seg[s].kind == RSP_SEG_FIR) { ++nfir; fir_idx = s; }
            else ++nmf;
        }
        ok = nfir <= 1 && nmf >= 1;
        int first = 1;
        for (int s = 0; s < p.nseg && ok; ++s) {
            if (pc.seg[s].kind != RSP_SEG_MF) continue;
            rsp::PcMfArgs a;
            std::memset(&a, 0, sizeof(a));
            a.R = (int)p.R;
            a.R_out = (int)p.R_out;
            a.mf = pc.seg[s];
            if (first) {
                a.do_fir = fir_idx >= 0;
                if (a.do_fir) a.fir = pc.seg[fir_idx];
                a.nzero = pc.nzero;
                for (int z = 0; z < pc.nzero; ++z) {
                    a.zero_lo[z] = pc.zero_lo[z];
                    a.zero_hi[z] = pc.zero_hi[z];
                }
                if (!rsp::pc_mf_supported(a.mf.nfft, a.do_fir ? rsp::fir_stage_len(a.fir) : 0)) ok = false;
                first = 0;
            } else if (!rsp::pc_mf_supported(a.mf.nfft, 0)) {
                ok = false;
            }
            pc_prune_counts(a);
            ctx->pc_mf_whole.push_back(a);
            if (ok) {
                const int rc = pc_overlap_save(ctx, p.seg[s], a);
                if (rc) return bail(rc);
            }
            pc_prune_counts(a);
            ctx->pc_mf_split.push_back(a);
            ctx->pc_mf.push_back(a);
        }
        ctx->pc_v2 = ok;
        if (!ok) {
            ctx->pc_mf.clear();
            ctx->pc_mf_whole.clear();
            ctx->pc_mf_split.clear();
        }
    }

    // ---- MTD
    rsp::MtdArgs& m = ctx->mtd;
    ctx->V = V;
    ctx->beams = beams;
    m.P = (int)V;            // Doppler FFT length; pulses beyond pin are the zero padding
    m.pin = (int)p.P;
    m.beams = beams;
    m.R_out = (int)p.R_out;
    m.shift = p.fftshift ? (int)(V / 2) : 0;
    if (p.zero_ends > 0) {   // rows [V-n+1, V) and [0, n): a band wrapping through row 0
        m.z_lo = (int)(V - p.zero_ends + 1);
        m.z_hi = (int)(V + p.zero_ends);
    } else {
        zero_v_band(V, p.zero_v_div, &m.z_lo, &m.z_hi);
    }
    std::vector<double> w = make_window(p.window, p.window_beta, p.P);   // window(P), zero-padded
    std::vector<float> wf((size_t)V, 0.f);
    for (int64_t i = 0; i < p.P; ++i) wf[(size_t)i] = (float)w[(size_t)i];
    float* dw = nullptr;
    int rc = upload(ctx, wf, &dw);
    if (rc) return bail(rc);
    m.win = dw;
    if (bluestein) {
        // X[k] = c[k] sum_n (x[n] w[n] c[n]) conj(c[k-n]), c[n] = exp(-j pi n^2 / V): tables in
        // fp64 (n^2 reduced mod 2V so the phase stays exact), the chirp spectrum by FFT
        const int nf = rsp::mtd_bluestein_nf((int)V);
        auto chirp = [&](int64_t n) {
            const double ph = -M_PI * (double)((n * n) % (2 * V)) / (double)V;
            return cd(std::cos(ph), std::sin(ph));
        };
        std::vector<float2> bwc((size_t)nf, float2{0.f, 0.f}), bsp((size_t)nf);
        for (int64_t n = 0; n < V; ++n) {
            const cd z = w[(size_t)n] * chirp(n);
            bwc[(size_t)n] = float2{(float)z.real(), (float)z.imag()};
        }
        std::vector<cd> b((size_t)nf, cd(0, 0));
        for (int64_t n = 0; n < V; ++n) {
            b[(size_t)n] = std::conj(chirp(n));
            if (n) b[(size_t)(nf - n)] = std::conj(chirp(n));
        }
        fft_pow2(b);
        for (int i = 0; i < nf; ++i) bsp[(size_t)i] = float2{(float)(b[(size_t)i].real() / nf), (float)(b[(size_t)i].imag() / nf)};
        float2 *dbwc = nullptr, *dbsp = nullptr;
        if ((rc = upload(ctx, bwc, &dbwc))) return bail(rc);
        if ((rc = upload(ctx, bsp, &dbsp))) return bail(rc);
        m.bnf = nf;
        m.bwc = dbwc;
        m.bspec = dbsp;
        rc = twiddles(ctx, nf, &m.tw);
    } else {
        rc = twiddles(ctx, (int)V, &m.tw);
    }
    if (rc) return bail(rc);
    *out = ctx;
    return RSP_OK;
}

// MTD/fun_lss_pulse_compression.m:31 (also DMX_SignalProcessing_main_xzr.m:146)
static const double kFirTaps[35] = {-9, -7, -2, 10, 27, 40, 42, 24, -13, -57, -89, -86, -30, 77, 220, 364, 471, 511,
                                    471, 364, 220, 77, -30, -86, -89, -57, -13, 24, 42, 40, 27, 10, -2, -7, -9};

static int64_t colon_count(double a, double d, double b) {   // MATLAB a:d:b length
    const double q = (b - a) / d;
    const double r = std::floor(q + 0.5);
    return (std::fabs(q - r) < 1e-9 * (std::fabs(q) > 1 ? std::fabs(q) : 1.0) ? (int64_t)r : (int64_t)std::floor(q)) + 1;
}

static int64_t nextpow2(int64_t n) {
    int64_t p = 64;
    while (p < n) p <<= 1;
    return p;
}

int rsp_create_v2(rsp_ctx** out, int device, int64_t P, int64_t R, const int64_t point_prt[4], double fs,
                  double B, const double tao[3]) {
    if (!out || !point_prt || !tao || fs <= 0 || tao[1] <= 0 || tao[2] <= 0)
        return fail(nullptr, RSP_ERR_ARG, "rsp_create_v2: bad argument");
    const int64_t p1 = point_prt[1], p2 = point_prt[2], p3 = point_prt[3];
    if (p1 < 1 || p2 < 1 || p3 < 1 || p1 + p2 + p3 > R)
        return fail(nullptr, RSP_ERR_SHAPE, "rsp_create_v2: point_prt segments exceed R=%lld", (long long)R);
    const double ts = 1.0 / fs;
    std::vector<double> re[2], im[2];
    for (int k = 0; k < 2; ++k) {   // pulse2 (K = -B/tau2), pulse3 (K = +B/tau3): fun_MTD_produce.m:62-69
        const double tau = tao[k + 1], K = (k == 0 ? -B : B) / tau;
        const int64_t n = colon_count(-tau / 2, ts, tau / 2 - ts);
        re[k].resize((size_t)n);
        im[k].resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const double t = -tau / 2 + ts * (double)i;
            const double ph = 2.0 * M_PI * 0.5 * K * t * t;
            re[k][i] = std::cos(ph);
            im[k][i] = std::sin(ph);
        }
    }
    std::vector<double> taps(35);
    for (int i = 0; i < 35; ++i) taps[i] = kFirTaps[i] / 511.0;   // filter_coef / max (:32)
    rsp_params prm;
    std::memset(&prm, 0, sizeof(prm));
    prm.P = P;
    prm.R = R;
    prm.R_out = R;
    prm.nseg = 3;
    prm.window = RSP_WIN_KAISER;
    prm.window_beta = 8.0;
    prm.fftshift = 1;
    prm.zero_v_div = 150;
    rsp_pc_segment& a = prm.seg[0];
    a.kind = RSP_SEG_FIR;
    a.fir_shift = 17;   // round(mean(grpdelay(b))) of the symmetric 35-tap FIR (:47)
    a.in_start = 0;
    a.in_len = a.out_len = p1;
    a.scale = 1.0 / 1.2;
    a.coef_len = 35;
    a.coef_re = taps.data();
    const int64_t m3 = R - p1 - p2;
    for (int k = 0; k < 2; ++k) {
        rsp_pc_segment& g = prm.seg[k + 1];
        g.kind = RSP_SEG_MF;
        g.in_start = g.out_start = k == 0 ? p1 : p1 + p2;
        g.in_len = k == 0 ? p2 : m3;
        g.out_len = k == 0 ? p2 : p3;
        g.coef_len = (int64_t)re[k].size();
        g.nfft = nextpow2(g.in_len + g.coef_len - 1);
        g.scale = 1.0;
        g.coef_re = re[k].data();
        g.coef_im = im[k].data();
    }
    return rsp_create(out, device, &prm);
}

int rsp_create_legacy(rsp_ctx** out, int device, int64_t P, int64_t R, const double* pulse2_re,
                      const double* pulse2_im, int64_t n2, const double* pulse3_re, const double* pulse3_im,
                      int64_t n3) {
    if (!out || !pulse2_re || !pulse2_im || !pulse3_re || !pulse3_im || n2 < 1 || n3 < 1)
        return fail(nullptr, RSP_ERR_ARG, "rsp_create_legacy: bad argument");
    const int64_t p1 = 82, p2 = 242, p3 = R - 324;   // fun_MTD_produce.m:24-38 (legacy)
    if (p3 < 1) return fail(nullptr, RSP_ERR_SHAPE, "rsp_create_legacy: R=%lld <= 324", (long long)R);
    std::vector<double> taps(35);
    for (int i = 0; i < 35; ++i) taps[i] = kFirTaps[i] / 511.0;   // filter_coef / max
    rsp_params prm;
    std::memset(&prm, 0, sizeof(prm));
    prm.P = P;
    prm.R = R;
    prm.R_out = R;
    prm.nseg = 3;
    prm.window = RSP_WIN_KAISER;
    prm.window_beta = 8.0;
    prm.fftshift = 1;
    prm.zero_v_div = 150;
    rsp_pc_segment& a = prm.seg[0];
    a.kind = RSP_SEG_FIR;
    a.fir_shift = 0;    // the legacy version keeps the FIR's group delay
    a.in_start = 0;
    a.in_len = a.out_len = p1;
    a.scale = 1.0 / 1.2;
    a.coef_len = 35;
    a.coef_re = taps.data();
    const double* re[2] = {pulse2_re, pulse3_re};
    const double* im[2] = {pulse2_im, pulse3_im};
    const int64_t n[2] = {n2, n3};
    const int64_t m3 = R - p1 - p2;
    for (int k = 0; k < 2; ++k) {
        rsp_pc_segment& g = prm.seg[k + 1];
        g.kind = RSP_SEG_MF;
        g.in_start = g.out_start = k == 0 ? p1 : p1 + p2;
        g.in_len = k == 0 ? p2 : m3;
        g.out_len = k == 0 ? p2 : p3;
        g.coef_len = n[k];
        g.nfft = nextpow2(g.in_len + g.coef_len - 1);
        g.scale = 1.0;
        g.coef_re = re[k];
        g.coef_im = im[k];
    }
    return rsp_create(out, device, &prm);
}

int rsp_set_streams(rsp_ctx* ctx, int32_t n) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_set_streams: null ctx");
    if (n < 0 || n > 4) return fail(ctx, RSP_ERR_ARG, "rsp_set_streams: n must be 0..4");
    ctx->nstreams = n;   // 0: the mode-dependent default
    return RSP_OK;
}

int rsp_set_chunk(rsp_ctx* ctx, int64_t cpis) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_set_chunk: null ctx");
    if (cpis < 0) return fail(ctx, RSP_ERR_ARG, "rsp_set_chunk: negative chunk");
    ctx->chunk = cpis;
    if (cpis > 0) ctx->nlane_cpis = 0;   // an explicit chunk means equal chunks
    return RSP_OK;
}

int rsp_set_lane_chunks(rsp_ctx* ctx, const int64_t* cpis, int32_t n) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_set_lane_chunks: null ctx");
    if (n < 0 || n > rsp::kMaxLanes || (n > 0 && !cpis))
        return fail(ctx, RSP_ERR_ARG, "rsp_set_lane_chunks: n must be 0..%d with a size list", rsp::kMaxLanes);
    for (int i = 0; i < n; ++i)
        if (cpis[i] < 1) return fail(ctx, RSP_ERR_ARG, "rsp_set_lane_chunks: chunk %d is %lld CPIs", i, (long long)cpis[i]);
    for (int i = 0; i < n; ++i) ctx->lane_cpis[i] = cpis[i];
    ctx->nlane_cpis = n;
    return RSP_OK;
}

// The default two-lane split of an unset chunk of cu CPIs (run_chain_body): *a == *b keeps the
// equal chunks.  Dev A/B: RSP_LANE_SPLIT="a,b" in CPIs (read once), "0" for equal chunks.
static void default_lane_split(int64_t cu, int64_t* a, int64_t* b) {
    static const struct Env { int64_t a = -1, b = -1; Env() {
        const char* v = getenv("RSP_LANE_SPLIT");
        if (v && *v) { long long x = 0, y = 0; const int k = sscanf(v, "%lld,%lld", &x, &y); a = x; b = k == 2 ? y : x; }
    } } env;
    if (env.a >= 0) {
        *a = env.a;
        *b = env.b;
        return;
    }
    *a = *b = cu;   // (no unequal pair beat the equal chunks at c3: DESIGN.md §7e)
}


bool set_device(rsp_ctx* ctx) { return hipSetDevice(ctx->device) == hipSuccess; }

static int64_t chunk_of(const rsp_ctx* ctx, int64_t batch) {
    int64_t c = ctx->chunk;
    if (c <= 0) {
        const int64_t per = (ctx->V > ctx->beams * ctx->p.P ? ctx->V : ctx->beams * ctx->p.P) * ctx->p.R_out * 8;
        c = (64ll << 20) / (per > 0 ? per : 1);
        if (c < 1) c = 1;
    }
    if (c > batch) c = batch;
    if (c > 65535) c = 65535;
    return c;
}

// CFAR argument blocks from the public struct; validates like MATLAB would fail.
static int build_cfar(rsp_ctx* ctx, const rsp_cfar_params* cf, int64_t V, int64_t R,
                      rsp::CfarVArgs* cv, rsp::CfarRArgs* cr) {
    if (cf->refV < 1 || cf->saveV < 0 || cf->refR < 1 || cf->saveR < 0)
        return fail(ctx, RSP_ERR_ARG, "CFAR: reference cells must be >= 1 and guard cells >= 0");
    if (cf->M0 < 0 || 2 * (int64_t)cf->M0 + 1 > V)
        return fail(ctx, RSP_ERR_ARG, "CFAR: M0=%d leaves no rows of %lld", cf->M0, (long long)V);
    if (cf->nseg < 0 || cf->nseg > RSP_MAX_SEG) return fail(ctx, RSP_ERR_ARG, "CFAR: bad nseg %d", cf->nseg);
    const int lo = cf->M0 + 1, hi = (int)V - cf->M0;
    if (hi - lo < 2 * (cf->saveV + cf->refV))
        return fail(ctx, RSP_ERR_CFAR_WINDOW,
                    "CFAR: %d Doppler cells after stripping M0 rows < 2*(guard+ref)=%d "
                    "(Function_CFAR1D_sub would index out of range)",
                    hi - lo, 2 * (cf->saveV + cf->refV));
    int nseg = cf->nseg;
    int64_t slo[RSP_MAX_SEG], shi[RSP_MAX_SEG];
    if (nseg == 0) {
        nseg = 1;
        slo[0] = 0;
        shi[0] = R;
    } else {
        for (int s = 0; s < nseg; ++s) {
            slo[s] = cf->seg_lo[s];
            shi[s] = cf->seg_hi[s];
            if (slo[s] < 0 || shi[s] > R || shi[s] <= slo[s])
                return fail(ctx, RSP_ERR_ARG, "CFAR: segment %d [%lld,%lld) outside [0,%lld)", s,
                            (long long)slo[s], (long long)shi[s], (long long)R);
            for (int q = 0; q < s; ++q)
                if (slo[s] < shi[q] && slo[q] < shi[s]) return fail(ctx, RSP_ERR_ARG, "CFAR: segments overlap");
        }
    }
    if (cf->rFlag && cf->saveR + cf->refR + 2 > 32)
        return fail(ctx, RSP_ERR_UNSUPPORTED, "CFAR: range guard+ref = %d > 30 not built", cf->saveR + cf->refR);
    if (cf->rFlag)
        for (int s = 0; s < nseg; ++s)
            if (shi[s] - slo[s] < 2 * (cf->saveR + cf->refR))
                return fail(ctx, RSP_ERR_CFAR_WINDOW,
                            "CFAR: range segment %d has %lld cells < 2*(guard+ref)=%d", s,
                            (long long)(shi[s] - slo[s]), 2 * (cf->saveR + cf->refR));
    int cz_lo, cz_hi;
    zero_v_band(V, cf->zero_v_div, &cz_lo, &cz_hi);
    std::memset(cv, 0, sizeof(*cv));
    cv->enabled = 1;
    cv->lo = lo;
    cv->hi = hi;
    cv->ref = cf->refV;
    cv->save = cf->saveV;
    cv->method = cf->methodV;
    cv->T = (float)cf->TV;
    cv->Tr = (float)(cf->TV / cf->refV);
    cv->cz_lo = cz_lo;
    cv->cz_hi = cz_hi;
    cv->nseg = nseg;
    std::memset(cr, 0, sizeof(*cr));
    cr->V = (int)V;
    cr->R = (int)R;
    cr->lo = lo;
    cr->hi = hi;
    cr->rflag = cf->rFlag ? 1 : 0;
    cr->ref = cf->refR;
    cr->save = cf->saveR;
    cr->method = cf->methodR;
    cr->T = (float)cf->TR;
    cr->Tr = (float)(cf->TR / cf->refR);
    cr->cz_lo = cz_lo;
    cr->cz_hi = cz_hi;
    cr->nseg = nseg;
    for (int s = 0; s < nseg; ++s) {
        cv->seg_lo[s] = cr->seg_lo[s] = (int)slo[s];
        cv->seg_hi[s] = cr->seg_hi[s] = (int)shi[s];
    }
    return RSP_OK;
}


// Order this call's use of the context scratch after the previous call's (on any stream).
int rsp::scratch_acquire(rsp_ctx* ctx, hipStream_t s) {
    if (ctx->scratch_pending) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_scratch, 0));
    return RSP_OK;
}
int rsp::scratch_release(rsp_ctx* ctx, hipStream_t s) {
    if (!ctx->ev_scratch) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_scratch, hipEventDisableTiming));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_scratch, s));
    ctx->scratch_pending = true;
    return RSP_OK;
}

static hipError_t run_pc(rsp_ctx* ctx, const void* ein, int dtype, float2* out, int64_t rows, hipStream_t s,
                         int slot, int64_t slot_rows);

// Run one kernel launch, bracketed by HIP events on `s` when profiling is on (every
// ctx->prof-th launch: a timing event costs the stream a few microseconds, so a sampled
// bracket keeps the measured region's throughput unchanged).
template <typename F>
static hipError_t timed(rsp_ctx* ctx, int k, hipStream_t s, F&& launch) {
    if (!ctx->prof) return launch();
    if (ctx->prof_tick++ % (uint64_t)ctx->prof != 0) return launch();
    if (ctx->nev == ctx->evs.size()) {
        rsp_ctx::Ev e{k, nullptr, nullptr};
        hipError_t r = hipEventCreate(&e.a);
        if (r == hipSuccess) r = hipEventCreate(&e.b);
        if (r != hipSuccess) return r;
        ctx->evs.push_back(e);
    }
    rsp_ctx::Ev& e = ctx->evs[ctx->nev++];
    e.k = k;
    hipError_t r = hipEventRecord(e.a, s);
    if (r != hipSuccess) return r;
    r = launch();
    if (r != hipSuccess) return r;
    return hipEventRecord(e.b, s);
}

static hipError_t run_pc_rows(rsp_ctx* ctx, const void* ein, int dtype, float2* out, int64_t rows, hipStream_t s);
// Pulse compression of `rows` echo rows into `out` ([rows][R_out]).  With a range concatenation
// (rsp_set_range_concat) the full-width PC rows land in cat_tmp slot `slot` (ensured by the caller:
// slot_rows * pc_w complex per slot, slot_rows >= rows) and the parts are gathered into `out` by
// 2-D copies on s.  The slot starts at its fixed capacity, not at this call's row count: a short
// last chunk on lane 1 would otherwise start inside lane 0's slot while lane 0 still uses it.
static hipError_t run_pc(rsp_ctx* ctx, const void* ein, int dtype, float2* out, int64_t rows, hipStream_t s,
                         int slot, int64_t slot_rows) {
    if (ctx->ncat == 0) return run_pc_rows(ctx, ein, dtype, out, rows, s);
    float2* full = (float2*)ctx->cat_tmp.p + (size_t)slot * (size_t)slot_rows * ctx->pc_w;
    hipError_t e = run_pc_rows(ctx, ein, dtype, full, rows, s);
    if (e != hipSuccess) return e;
    const size_t so = sizeof(float2);
    int64_t dst = 0;
    for (int i = 0; i < ctx->ncat; ++i) {
        e = hipMemcpy2DAsync(out + dst, (size_t)ctx->p.R_out * so, full + ctx->cat_src[i], (size_t)ctx->pc_w * so,
                             (size_t)ctx->cat_len[i] * so, (size_t)rows, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
        dst += ctx->cat_len[i];
    }
    return hipSuccess;
}
static int cat_ensure(rsp_ctx* ctx, int slots, int64_t rows) {
    return ctx->ncat ? ensure(ctx, ctx->cat_tmp, (size_t)slots * rows * ctx->pc_w * sizeof(float2)) : RSP_OK;
}

int rsp_set_range_concat(rsp_ctx* ctx, int32_t nparts, const int64_t* src_start, const int64_t* len) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_set_range_concat: null ctx");
    if (ctx->cfar_only) return fail(ctx, RSP_ERR_ARG, "rsp_set_range_concat: CFAR-only context");
    if (nparts < 0 || nparts > RSP_MAX_SEG || (nparts > 0 && (!src_start || !len)))
        return fail(ctx, RSP_ERR_ARG, "rsp_set_range_concat: bad part list (%d parts)", nparts);
    int64_t w = 0;
    for (int i = 0; i < nparts; ++i) {
        if (len[i] < 1 || src_start[i] < 0 || src_start[i] + len[i] > ctx->pc_w)
            return fail(ctx, RSP_ERR_ARG, "rsp_set_range_concat: part %d [%lld, +%lld) outside the %lld PC columns", i,
                        (long long)src_start[i], (long long)len[i], (long long)ctx->pc_w);
        w += len[i];
    }
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(ctx, hipDeviceSynchronize());   // no launch in flight still uses the old width
    ctx->ncat = nparts;
    for (int i = 0; i < nparts; ++i) {
        ctx->cat_src[i] = src_start[i];
        ctx->cat_len[i] = len[i];
    }
    ctx->p.R_out = nparts > 0 ? w : ctx->pc_w;
    ctx->mtd.R_out = (int)ctx->p.R_out;
    return RSP_OK;
}

// The specialised path's launches as run_pc_rows issues them and rsp_pc_plan reports them: both
// matched filters in one launch where the pair is built, else one launch per segment.
static bool pc_fused(const rsp_ctx* ctx) {
    return ctx->pc_mf.size() == 2 && rsp::pc_pair_supported(ctx->pc_mf[0].mf.nfft, ctx->pc_mf[1].mf.nfft);
}
static rsp::PcMfArgs pc_launch_args(const rsp_ctx* ctx, size_t i, int64_t rows) {
    rsp::PcMfArgs a = ctx->pc_mf[i];
    a.rows = (int)rows;
    if (!ctx->pc_prune) a.zin = a.zout = 0;
    return a;
}

// Rows per long-row workgroup slot asked of the launcher: rsp_set_pc_rows, else the library default.
// Dev A/B: RSP_PC_ROWS=1|2|4 replaces the default (read once).
static int pc_rows_want(const rsp_ctx* ctx) {
    static const int dflt = [] {
        const char* v = getenv("RSP_PC_ROWS");
        const int n = v ? atoi(v) : 0;
        return rsp::pc_rows_valid(n) ? n : rsp::kPcRowsDefault;
    }();
    return ctx->pc_rows ? ctx->pc_rows : dflt;
}

static hipError_t run_pc_rows(rsp_ctx* ctx, const void* ein, int dtype, float2* out, int64_t rows, hipStream_t s) {
    const int want = ctx->pc_v2 ? pc_rows_want(ctx) : 1;
    if (!ctx->pc_v2)
        return timed(ctx, RSP_K_PC, s, [&] { return rsp::launch_pc(ein, dtype, out, rows, ctx->pc, ctx->pc_lds, s); });
    if (pc_fused(ctx)) {
        const rsp::PcMfArgs a1 = pc_launch_args(ctx, 0, rows), a2 = pc_launch_args(ctx, 1, rows);
        return timed(ctx, RSP_K_PC, s, [&] { return rsp::launch_pc_mf(ein, dtype, out, a1, &a2, want, s); });
    }
    for (size_t i = 0; i < ctx->pc_mf.size(); ++i) {
        const rsp::PcMfArgs a = pc_launch_args(ctx, i, rows);
        hipError_t e = timed(ctx, RSP_K_PC, s, [&] { return rsp::launch_pc_mf(ein, dtype, out, a, nullptr, want, s); });
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

int rsp_pc_plan(rsp_ctx* ctx, rsp_pc_plan_t* out, int32_t n) {
    if (!ctx || !out) return fail(ctx, RSP_ERR_ARG, "rsp_pc_plan: null argument");
    if (ctx->cfar_only) return fail(ctx, RSP_ERR_ARG, "rsp_pc_plan: CFAR-only context");
    if (n < 0 || n > RSP_MAX_SEG || (size_t)n < ctx->pc_mf.size())
        return fail(ctx, RSP_ERR_ARG, "rsp_pc_plan: room for %d segments, the context has %d", n, (int)ctx->pc_mf.size());
    std::memset(out, 0, sizeof(*out));
    out->specialised = ctx->pc_v2 ? 1 : 0;
    if (!ctx->pc_v2) return RSP_OK;
    out->nmf = (int32_t)ctx->pc_mf.size();
    out->fused = pc_fused(ctx) ? 1 : 0;
    for (size_t i = 0; i < ctx->pc_mf.size(); ++i) {
        const rsp::PcMfArgs a = pc_launch_args(ctx, i, 1);
        rsp_pc_plan_seg& g = out->seg[i];
        g.nfft = a.mf.nfft;
        g.nsub = a.nsub;
        g.sub_step = a.sub_step;
        g.zin = a.zin;
        g.zout = a.zout;
        g.fir = a.do_fir;
    }
    if (out->fused) {
        const rsp::PcMfArgs a1 = pc_launch_args(ctx, 0, 1), a2 = pc_launch_args(ctx, 1, 1);
        out->prune = rsp::pc_prune_select(a1, &a2);
    } else {   // one launch per segment
        for (size_t i = 0; i < ctx->pc_mf.size(); ++i) {
            const rsp::PcMfArgs a = pc_launch_args(ctx, i, 1);
            if (const int pr = rsp::pc_prune_select(a, nullptr)) out->prune = pr;
        }
    }
    return RSP_OK;
}

int rsp_profile(rsp_ctx* ctx, int32_t enable) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_profile: null ctx");
    if (enable < 0) return fail(ctx, RSP_ERR_ARG, "rsp_profile: enable %d < 0", enable);
    ctx->prof = enable;
    ctx->prof_tick = 0;
    ctx->nev = 0;
    for (int k = 0; k < RSP_NKERNELS; ++k) {
        ctx->prof_ms[k] = 0;
        ctx->prof_n[k] = 0;
    }
    return RSP_OK;
}

int rsp_profile_read_n(rsp_ctx* ctx, double* ms, int64_t* launches, int32_t n) {
    if (!ctx || !ms || !launches || n < 0) return fail(ctx, RSP_ERR_ARG, "rsp_profile_read_n: bad argument");
    for (size_t i = 0; i < ctx->nev; ++i) {
        rsp_ctx::Ev& e = ctx->evs[i];
        HIP_TRY(ctx, hipEventSynchronize(e.b));
        float t = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&t, e.a, e.b));
        ctx->prof_ms[e.k] += t;
        ctx->prof_n[e.k] += 1;
    }
    ctx->nev = 0;
    for (int k = 0; k < n && k < RSP_NKERNELS; ++k) {
        ms[k] = ctx->prof_ms[k];
        launches[k] = ctx->prof_n[k];
    }
    return RSP_OK;
}

// the ABI-3 form: exactly the four kernel ids that header declared (RSP_K_PC .. RSP_K_CFAR_V)
int rsp_profile_read(rsp_ctx* ctx, double* ms, int64_t* launches) {
    if (!ctx || !ms || !launches) return fail(ctx, RSP_ERR_ARG, "rsp_profile_read: null argument");
    return rsp_profile_read_n(ctx, ms, launches, 4);
}

int rsp_pc_dev(rsp_ctx* ctx, const void* d_echo, int32_t dtype, int64_t batch, void* d_pc, void* stream) {
    if (!ctx || !d_echo || !d_pc || batch < 0) return fail(ctx, RSP_ERR_ARG, "rsp_pc_dev: bad argument");
    if (ctx->cfar_only) return fail(ctx, RSP_ERR_ARG, "context was created for CFAR only (params == NULL)");
    if (dtype != RSP_C64 && dtype != RSP_C32F16) return fail(ctx, RSP_ERR_ARG, "rsp_pc_dev: dtype %d", dtype);
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    if (ctx->ncat == 0) {
        HIP_TRY(ctx, run_pc(ctx, d_echo, dtype, (float2*)d_pc, batch * ctx->p.P, (hipStream_t)stream, 0, 0));
        return RSP_OK;
    }
    // the concatenation stages full-width rows in the context's scratch
    hipStream_t s = (hipStream_t)stream;
    int rc = scratch_acquire(ctx, s);
    if (rc) return rc;
    if ((rc = cat_ensure(ctx, 1, batch * ctx->p.P))) return rc;
    HIP_TRY(ctx, run_pc(ctx, d_echo, dtype, (float2*)d_pc, batch * ctx->p.P, s, 0, batch * ctx->p.P));
    return scratch_release(ctx, s);
}

int rsp_set_pc_split(rsp_ctx* ctx, int32_t enable) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_set_pc_split: null ctx");
    if (ctx->cfar_only) return fail(ctx, RSP_ERR_ARG, "rsp_set_pc_split: CFAR-only context");
    if (!ctx->pc_v2)   // the generic PC path has no split to select
        return fail(ctx, RSP_ERR_UNSUPPORTED, "rsp_set_pc_split: this context has no specialised PC path");
    const std::vector<rsp::PcMfArgs>& src = enable ? ctx->pc_mf_split : ctx->pc_mf_whole;
    for (size_t i = 0; i < ctx->pc_mf.size() && i < src.size(); ++i) {
        const float* gain = ctx->pc_mf[i].gain;   // the fused pre-filter stays as set
        ctx->pc_mf[i] = src[i];
        ctx->pc_mf[i].gain = gain;
    }
    return RSP_OK;
}

int rsp_set_pc_prune(rsp_ctx* ctx, int32_t enable) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_set_pc_prune: null ctx");
    if (ctx->cfar_only) return fail(ctx, RSP_ERR_ARG, "rsp_set_pc_prune: CFAR-only context");
    if (!ctx->pc_v2)   // the generic PC path has no pruned instances
        return fail(ctx, RSP_ERR_UNSUPPORTED, "rsp_set_pc_prune: this context has no specialised PC path");
    ctx->pc_prune = enable != 0;
    return RSP_OK;
}

int rsp_set_pc_rows(rsp_ctx* ctx, int32_t n) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_set_pc_rows: null ctx");
    if (ctx->cfar_only) return fail(ctx, RSP_ERR_ARG, "rsp_set_pc_rows: CFAR-only context");
    if (!ctx->pc_v2)   // the generic PC path runs one row per workgroup
        return fail(ctx, RSP_ERR_UNSUPPORTED, "rsp_set_pc_rows: this context has no specialised PC path");
    if (n != 0 && !rsp::pc_rows_valid(n)) return fail(ctx, RSP_ERR_ARG, "rsp_set_pc_rows: %d is not 0, 1, 2 or 4", (int)n);
    ctx->pc_rows = n;
    return RSP_OK;
}

// What the next launches will use: the launcher's own choice (pc_rows_select) for each launch of
// run_pc_rows, the largest of them where a context has several.
int rsp_get_pc_rows(rsp_ctx* ctx) {
    if (!ctx || ctx->cfar_only || !ctx->pc_v2) return 1;
    const int want = pc_rows_want(ctx);
    if (pc_fused(ctx)) {
        const rsp::PcMfArgs a1 = pc_launch_args(ctx, 0, 1), a2 = pc_launch_args(ctx, 1, 1);
        return rsp::pc_rows_select(a1, &a2, want);
    }
    int rows = 1;
    for (size_t i = 0; i < ctx->pc_mf.size(); ++i) {
        const rsp::PcMfArgs a = pc_launch_args(ctx, i, 1);
        const int r = rsp::pc_rows_select(a, nullptr, want);
        if (r > rows) rows = r;
    }
    return rows;
}

int rsp_set_prefilter(rsp_ctx* ctx, const float* gain, int32_t mti_lag) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_set_prefilter: null ctx");
    if (ctx->cfar_only) return fail(ctx, RSP_ERR_ARG, "rsp_set_prefilter: CFAR-only context");
    if (mti_lag < 0) return fail(ctx, RSP_ERR_ARG, "rsp_set_prefilter: negative MTI lag %d", mti_lag);
    if (gain && !ctx->pc_v2)
        return fail(ctx, RSP_ERR_UNSUPPORTED, "rsp_set_prefilter: the fused gain needs the per-segment PC kernels");
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(ctx, hipDeviceSynchronize());   // no launch in flight still reads the old gains
    const float* d_gain = nullptr;
    if (gain) {
        const size_t bytes = (size_t)ctx->p.R * sizeof(float);
        const int rc = ensure(ctx, ctx->pf_gain, bytes);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpy(ctx->pf_gain.p, gain, bytes, hipMemcpyHostToDevice));
        d_gain = (const float*)ctx->pf_gain.p;
    }
    for (rsp::PcMfArgs& a : ctx->pc_mf) a.gain = d_gain;
    ctx->mtd.mti_lag = mti_lag;
    return RSP_OK;
}

// The chain over `units` on stream s.  win == 0: a unit is one CPI ([P][R] input rows).
// win > 0: a unit is a frame pair (n, n+1) of a frame-contiguous input holding units + 1
// frames, producing `win` windowed CPIs (MtdArgs::win); a chunk computes the PC of its
// frames plus the look-ahead frame once, and every window reads its rows from that PC.
// Where a chunk's range stage (executeCFAR's range test of the Doppler hits) runs:
//   2 (default): grouped -- the range stages of up to kRangeGroup consecutive chunks of a lane run
//     as one launch behind the group's last MTD; the MTD records hit indices relative to the
//     group's first output cell (MtdArgs::cell_off).  Needs the caller's RDM (internal RDM slots
//     are reused) and a group span inside the range kernels' 2 GiB buffer window.
//   0: fused -- the stage rides in the next MTD launch on the lane (RangeJob57: gathers issued with
//     the tile loads); the fallback when grouping does not apply.
//   1: a standalone launch behind every chunk's MTD.
// Measured (profiles/r05/ab/range_stage_grouping.txt): the fused job costs the MTD ~10 % at c3
// even with 0.28 % hits; groups of 8-32 chunks: c3 +2 %, c5 +1.5-2.6 %, bit-identical; a launch
// per chunk: c3 -1 %.  Dev A/B: environment RSP_RANGE_MODE / RSP_RANGE_GROUP (read once).
static constexpr int kRangeGroup = 16;
static constexpr uint64_t kRangeGroupBytes = 1ull << 30;   // hit-list slots of one call's groups
static int range_mode() {
    static const int m = [] { const char* v = getenv("RSP_RANGE_MODE"); return v && *v ? atoi(v) : 2; }();
    return m;
}
static int range_group() {
    static const int g = [] { const char* v = getenv("RSP_RANGE_GROUP"); const int x = v && *v ? atoi(v) : kRangeGroup; return x < 1 ? 1 : x; }();
    return g;
}

// The chunk plan and the range-stage choices of one chain call over `units` (run_chain_body's
// arguments): run_chain_body launches by it and rsp_cfar_plan reports it.
struct ChainLayout {
    int64_t ocpi = 1;                 // output CPIs per unit
    rsp::ChunkPlan plan;
    size_t plane = 0;                 // output cells per CPI
    size_t cells = 0;                 // output cells per chunk slot
    size_t pcrows = 0;                // PC rows of the call's largest chunk
    int nreg[rsp::kMaxLanes] = {};    // hit-list regions of a lane's full chunk
    int reg = 0;                      // entries per region
    size_t nreg_all = 0;              // all lanes' regions together
    int rgrp = 1;                     // chunks per range-stage group
    bool grouped = false;             // the range stages run as one launch per group
    int spl = 2;                      // hit-list slots per lane
    bool fm = false;                  // the flag background is a memset before the MTD
};
static int chain_layout(rsp_ctx* ctx, int64_t units, int win, bool cfar, const rsp::CfarRArgs& cr, bool have_rdm,
                        bool have_flag, ChainLayout* L) {
    const int64_t P = ctx->p.P, Ro = ctx->p.R_out, V = ctx->V, NB = ctx->beams;
    const int64_t ocpi = win > 0 ? win : 1;               // output CPIs per unit
    L->ocpi = ocpi;
    int64_t cu = chunk_of(ctx, units * ocpi);              // CPIs per chunk
    // Default pipelines: 2 (PC of one chunk overlaps MTD / CFAR of the other); window mode 1 with
    // chunks of >= 32 frame pairs (look-ahead PC overhead <= 1/32, fewer launch tails): c4 114.9k
    // windows/s against 111.9k at 16 pairs and 106.5k at 8 (round 3); two pipelines of 8 pairs
    // lost (2 x 144 MiB of scratch overflows the Infinity Cache)
    const int nsd = ctx->nstreams > 0 ? ctx->nstreams : (win > 0 ? 1 : 2);
    if (win > 0) {
        cu = cu / ocpi;
        if (ctx->chunk > 0) {
            cu = cu > 0 ? cu : 1;                          // explicit chunk (rsp_set_chunk): as asked
        } else if (cu < 32) {
            // at least 32 pairs, but never more cells per chunk slot than the 32-bit hit
            // indices address (down to the old minimum and below for the largest windows)
            const int64_t fit = (int64_t)(0xffffffffull / ((uint64_t)ocpi * (uint64_t)V * (uint64_t)Ro));
            cu = 32 < fit ? 32 : (fit > cu ? fit : cu);
            if (cu < 1) cu = 1;
        }
    }
    if (cu > units) cu = units;
    // Chunk boundaries (rsp_chunkplan.h): chunk k covers units [cstart[k], cstart[k + 1]) on lane
    // k % ns; a lane's chunks are lcu[lane] units each, only the call's final chunk is short.
    // Equal chunks of cu units, unless rsp_set_lane_chunks gave the lanes their own sizes (which
    // also sets the lane count) or the default two-lane split applies (kLaneSplit*).
    int64_t lcu[rsp::kMaxLanes] = {cu, cu, cu, cu};
    int nlanes = nsd;
    if (win == 0 && ctx->nlane_cpis > 0) {
        nlanes = ctx->nlane_cpis;
        for (int i = 0; i < nlanes; ++i) lcu[i] = ctx->lane_cpis[i] < 65535 ? ctx->lane_cpis[i] : 65535;
    } else if (win == 0 && ctx->chunk <= 0 && nsd == 2) {
        int64_t a = 0, b = 0;
        default_lane_split(cu, &a, &b);
        if (rsp::lane_split_applies(units, a, b)) {
            lcu[0] = a;
            lcu[1] = b;
        }
    }
    L->plan = rsp::plan_chunks(units, lcu, nlanes);
    const rsp::ChunkPlan& plan = L->plan;
    const int ns = plan.ns;
    const size_t plane = (size_t)V * Ro;                  // output cells per CPI
    L->plane = plane;
    // concat staging and internal RDM slots are sized by the call's largest chunk; a lane's PC
    // scratch slot by the lane's own (16 / 24 CPIs at c3: 160 MiB of scratch, not 192)
    const size_t cells = (size_t)plan.cap_max * ocpi * plane;       // output cells per chunk slot
    L->cells = cells;
    L->pcrows = (size_t)(plan.cap_max + (win > 0 ? 1 : 0)) * NB * P;
    // hit-list regions of a lane's full chunk (nreg[lane], each `reg` indices: the region is one MTD
    // workgroup's cells, whatever the chunk size), and all lanes' together
    if (cfar) {
        // fused range stage: per-lane hit lists, one region per MTD workgroup sized to its
        // cells (no overflow, no global atomics), and per-workgroup counts
        if (cells > 0xffffffffull) return fail(ctx, RSP_ERR_UNSUPPORTED, "chunk too large for 32-bit hit indices");
        // two slots per lane: chunk k's list is read by the next MTD launch on its lane while
        // that launch fills the other slot
        for (int l = 0; l < ns; ++l) {
            rsp::mtd_regions((int)V, (int)Ro, (int)(plan.cap[l] * ocpi), &L->nreg[l], &L->reg, (int)NB);
            L->nreg_all += (size_t)L->nreg[l];
        }
    }
    // grouped range stages (range_mode 2): a group's outputs must stay inside the range kernels'
    // 2 GiB buffer window, and the RDM must be the caller's (internal RDM slots are reused)
    int rgrp = range_group();
    if (cfar && L->nreg_all > 0) {   // the groups' hit-list slots within kRangeGroupBytes
        const uint64_t round_bytes = (uint64_t)L->nreg_all * (uint64_t)L->reg * 4u;   // one slot of every lane
        const uint64_t fit = kRangeGroupBytes / round_bytes;
        if ((uint64_t)rgrp > fit) rgrp = fit > 0 ? (int)fit : 1;
    }
    L->rgrp = rgrp;
    // a lane's group spans rgrp - 1 whole rounds over the lanes plus its own last chunk
    L->grouped = cfar && cr.rflag && have_rdm && range_mode() == 2 && rgrp > 1 &&
                 ((uint64_t)(rgrp - 1) * (uint64_t)plan.period * ocpi * plane + (uint64_t)cells) * 4u <
                     0x80000000ull;   // (kOob, rsp_buf.h)
    // hit-list slots per lane: grouped, a group's range launch is stream-ordered before the next
    // group's first MTD on the lane, so the next group reuses the slots
    L->spl = L->grouped ? rgrp : 2;
    // The flag background: the MTD kernels' own stores, except for big chunks of long tiles: there a
    // memset of the chunk's flag plane on the lane before its MTD (a streaming fill) beats the tiles'
    // 16-byte row-segment stores (tiles of P >= 256 are 16 bins wide).  c4 (one 268 MB chunk per step): MTD 649 -> 572 us, +4.3 %;
    // c3 (32-bin tiles, 8 MiB chunks) -2.8 %, c5 (8 MiB chunks) neutral
    // (profiles/r05/ab/flag_memset.txt).  Dev A/B: RSP_FLAG_MEMSET 0 / 1 forces it off / on.
    static const int fenv = [] { const char* v = getenv("RSP_FLAG_MEMSET"); return v && *v ? atoi(v) : -1; }();
    L->fm = cfar && cr.rflag && have_flag &&
            (fenv >= 0 ? fenv == 1 : (V >= 256 && (uint64_t)cells >= (64ull << 20)));
    // (The fill on a side stream beside the chunk's PC, joined before the MTD, measured the same:
    // c4 133.8k vs 134.2k windows/s, three interleaved pairs, bit-identical -- the fill and the
    // PC share the HBM; profiles/r06/c4/flag_memset_side.txt.)
    return RSP_OK;
}

// RSP_RANGE_MODE=1: a hit-list launch behind every chunk's MTD (where grouping does not apply)
static bool range_per_chunk(const ChainLayout& L) { return !L.grouped && range_mode() == 1; }

static int run_chain_body(rsp_ctx* ctx, const void* d_echo, int32_t dtype, int64_t units, int win,
                          const rsp_cfar_params* cfar, float* d_rdm, uint8_t* d_flag, uint8_t* d_flagV,
                          float* d_diff, hipStream_t s, bool pc_input) {
    const int64_t P = ctx->p.P, R = ctx->p.R, Ro = ctx->p.R_out, V = ctx->V, NB = ctx->beams;
    const size_t esz = dtype == RSP_C64 ? 8 : 4;
    rsp::MtdArgs m = ctx->mtd;
    rsp::CfarRArgs cr{};
    if (cfar) {
        int rc = build_cfar(ctx, cfar, V, Ro, &m.cv, &cr);
        if (rc) return rc;
    } else {
        m.cv.enabled = 0;
    }
    m.nwin = win;
    for (int i = 0; i < win; ++i) m.win_start[i] = (int)mround((double)i * P / win);
    ChainLayout L;
    int rc = chain_layout(ctx, units, win, cfar != nullptr, cr, d_rdm != nullptr, d_flag != nullptr, &L);
    if (rc) return rc;
    const int64_t ocpi = L.ocpi;                           // output CPIs per unit
    const rsp::ChunkPlan& plan = L.plan;
    const std::vector<int64_t>& cstart = plan.cstart;
    const int64_t nchunks = plan.nchunks();
    const int ns = plan.ns;
    const size_t plane = L.plane, cells = L.cells, pcrows = L.pcrows;
    const int* nreg = L.nreg;
    const int reg = L.reg, rgrp = L.rgrp, spl = L.spl;
    const size_t nreg_all = L.nreg_all;
    const bool grouped = L.grouped, fm = L.fm;
    size_t pcoff[rsp::kMaxLanes + 1] = {};   // first PC scratch row of each lane's slot
    for (int l = 0; l < ns; ++l) pcoff[l + 1] = pcoff[l] + (size_t)(plan.cap[l] + (win > 0 ? 1 : 0)) * NB * P;
    rc = pc_input ? RSP_OK : ensure(ctx, ctx->scratch_pc, pcoff[ns] * Ro * sizeof(float2));
    if (rc) return rc;
    if (!pc_input && (rc = cat_ensure(ctx, ns, (int64_t)pcrows))) return rc;
    // lane l's slots start behind those of the lanes before it, each lane's sized by its own regions
    size_t hbase[rsp::kMaxLanes] = {};
    for (int l = 1; l < ns; ++l) hbase[l] = hbase[l - 1] + (size_t)spl * nreg[l - 1];
    if (cfar) {
        rc = ensure(ctx, ctx->hit_list, (size_t)spl * nreg_all * reg * sizeof(uint32_t));
        if (rc) return rc;
        rc = ensure(ctx, ctx->hit_ctr, (size_t)spl * nreg_all * sizeof(uint32_t));
        if (rc) return rc;
    }
    if (!d_rdm) {   // internal RDM: two slots per lane for the same reason
        rc = ensure(ctx, ctx->tmp_rdm, (size_t)2 * ns * cells * sizeof(float));
        if (rc) return rc;
    }
    // the MTD kernels write the flag plane's zero background with the Doppler stage (every cell
    // of a CPI belongs to one MTD thread), and the range stage, stream-ordered after that
    // chunk's MTD launch, writes the 1s: no separate fill pass -- except where chain_layout
    // chose the memset (fm)
    m.flag_zero = fm ? 0 : 1;
    // Chunk k runs on lane k % ns (lane 0 = the caller's stream), each lane with its own
    // scratch slot, so PC of one chunk overlaps MTD / CFAR of the previous one.  The lanes
    // fork from and join back into the caller's stream.
    hipStream_t lanes[4] = {s, nullptr, nullptr, nullptr};
    if (ns > 1) {
        if (!ctx->ev_fork) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, s));
        for (int i = 1; i < ns; ++i) {
            if (!ctx->aux[i - 1]) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->aux[i - 1], hipStreamNonBlocking));
            if (!ctx->ev_join[i - 1]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_join[i - 1], hipEventDisableTiming));
            lanes[i] = ctx->aux[i - 1];
            HIP_TRY(ctx, hipStreamWaitEvent(lanes[i], ctx->ev_fork, 0));
        }
    }
    // A chunk's range stage (its hit list) runs inside the next MTD launch on its lane, so the
    // lane timeline carries no separate small kernel; a lane's last chunk gets its own launch.
    struct Pending {
        int nreg = 0, reg = 0;
        const float* rdm = nullptr;
        uint8_t* flag = nullptr;
        const uint32_t* hits = nullptr;
        const uint32_t* counts = nullptr;
    } pend[4];
    for (int64_t k = 0; k < nchunks; ++k) {
        const int64_t u0 = cstart[(size_t)k];
        const int64_t n = cstart[(size_t)k + 1] - u0;
        const int64_t ncpi = n * ocpi;                     // CPIs this chunk produces
        const size_t o0 = (size_t)u0 * ocpi * plane;      // output offset
        const int lane = (int)(k % ns);
        const int64_t j = k / ns;                          // the chunk's index on its lane
        // first region of the chunk's hit-list slot: double-buffered per lane (grouped: one group)
        const size_t hslot = hbase[lane] + (size_t)(j % spl) * nreg[lane];
        const int64_t jg0 = j - j % rgrp;                  // grouped: the group's first chunk on the lane
        const size_t og = grouped ? (size_t)cstart[(size_t)(lane + ns * jg0)] * ocpi * plane : o0;
        hipStream_t ls = lanes[lane];
        const char* ein = (const char*)d_echo + (size_t)u0 * NB * P * R * esz;
        float* rdm = d_rdm ? d_rdm + o0 : (float*)ctx->tmp_rdm.p + (lane * 2 + (int)(j & 1)) * cells;
        uint8_t* fv = (cfar && d_flagV) ? d_flagV + o0 : nullptr;
        float2* pcs;
        if (pc_input) {   // d_echo already holds pulse-compressed rows [units][beams][P][R_out]
            pcs = (float2*)d_echo + (size_t)u0 * NB * P * Ro;
        } else {
            pcs = (float2*)ctx->scratch_pc.p + pcoff[lane] * Ro;
            HIP_TRY(ctx, run_pc(ctx, ein, dtype, pcs, (n + (win > 0 ? 1 : 0)) * NB * P, ls, lane, (int64_t)pcrows));
        }
        m.diff = d_diff ? d_diff + o0 : nullptr;
        m.prev_nregions = 0;
        m.cell_off = (uint32_t)(o0 - og);   // hit indices relative to the group's first cell (else 0)
        if (cfar) {
            m.flag = d_flag + o0;
            m.rflag = cr.rflag;
            m.hits = (uint32_t*)ctx->hit_list.p + hslot * reg;
            m.hit_count = (uint32_t*)ctx->hit_ctr.p + hslot;
            const Pending& pv = pend[lane];
            if (pv.nreg > 0 && !grouped) {
                m.prev_rdm = pv.rdm;
                m.prev_flag = pv.flag;
                m.prev_hits = pv.hits;
                m.prev_count = pv.counts;
                m.prev_nregions = pv.nreg;
                m.prev_region = pv.reg;
                m.prev_cr = cr;
            }
        }
        if (fm) HIP_TRY(ctx, hipMemsetAsync(d_flag + o0, 0, (size_t)ncpi * plane, ls));
        HIP_TRY(ctx, timed(ctx, RSP_K_MTD, ls, [&] { return rsp::launch_mtd(pcs, rdm, fv, (int)ncpi, m, ls); }));
        if (cfar && cr.rflag) {
            Pending& pv = pend[lane];
            rsp::mtd_regions((int)V, (int)Ro, (int)ncpi, &pv.nreg, &pv.reg, (int)NB);   // this chunk's workgroups
            pv.rdm = rdm;
            pv.flag = m.flag;
            pv.hits = m.hits;
            pv.counts = m.hit_count;
            if (grouped) {   // the group's range stages, one launch behind its last MTD
                const bool last = k + ns >= nchunks;
                if (j % rgrp == rgrp - 1 || last) {
                    const size_t s0 = hbase[lane] + (size_t)(jg0 % spl) * nreg[lane];
                    const int nr = (int)(j - jg0) * nreg[lane] + pv.nreg;   // the lane's full chunks, then this one's regions
                    HIP_TRY(ctx, timed(ctx, RSP_K_CFAR_R, ls, [&] {
                        return rsp::launch_cfar_hits(d_rdm + og, d_flag + og, (uint32_t*)ctx->hit_list.p + s0 * reg,
                                                     (uint32_t*)ctx->hit_ctr.p + s0, nr, pv.reg, cr, ls);
                    }));
                }
                pv.nreg = 0;
            } else if (range_per_chunk(L)) {   // (dev A/B) the chunk's range stage as its own launch, now
                HIP_TRY(ctx, timed(ctx, RSP_K_CFAR_R, ls, [&] {
                    return rsp::launch_cfar_hits(pv.rdm, pv.flag, pv.hits, pv.counts, pv.nreg, pv.reg, cr, ls);
                }));
                pv.nreg = 0;
            }
        }
    }
    for (int lane = 0; lane < ns; ++lane) {   // each lane's last chunk
        const Pending& pv = pend[lane];
        if (pv.nreg > 0)
            HIP_TRY(ctx, timed(ctx, RSP_K_CFAR_R, lanes[lane], [&] {
                return rsp::launch_cfar_hits(pv.rdm, pv.flag, pv.hits, pv.counts, pv.nreg, pv.reg, cr, lanes[lane]);
            }));
    }
    for (int i = 1; i < ns; ++i) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_join[i - 1], lanes[i]));
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_join[i - 1], 0));
    }
    return RSP_OK;
}

static int run_chain(rsp_ctx* ctx, const void* d_echo, int32_t dtype, int64_t units, int win,
                     const rsp_cfar_params* cfar, float* d_rdm, uint8_t* d_flag, uint8_t* d_flagV,
                     float* d_diff, hipStream_t s, bool pc_input = false) {
    int rc = scratch_acquire(ctx, s);
    if (rc) return rc;
    rc = run_chain_body(ctx, d_echo, dtype, units, win, cfar, d_rdm, d_flag, d_flagV, d_diff, s, pc_input);
    if (rc) return rc;
    return scratch_release(ctx, s);
}

static int check_chain_args(rsp_ctx* ctx, const char* fn, const void* d_echo, int32_t dtype, int64_t n,
                            const rsp_cfar_params* cfar, float* d_rdm, uint8_t* d_flag) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "%s: null ctx", fn);
    if (ctx->cfar_only) return fail(ctx, RSP_ERR_ARG, "context was created for CFAR only (params == NULL)");
    if (!d_echo || n < 0) return fail(ctx, RSP_ERR_ARG, "%s: bad input pointer/count", fn);
    if (dtype != RSP_C64 && dtype != RSP_C32F16)
        return fail(ctx, RSP_ERR_ARG, "%s: device dtype must be RSP_C64 or RSP_C32F16", fn);
    if (cfar && !d_flag) return fail(ctx, RSP_ERR_ARG, "%s: CFAR requested without d_flag", fn);
    if (!cfar && !d_rdm) return fail(ctx, RSP_ERR_ARG, "%s: no output requested", fn);
    return RSP_OK;
}

int rsp_pc_mtd_cfar_dev(rsp_ctx* ctx, const void* d_echo, int32_t dtype, int64_t batch,
                        const rsp_cfar_params* cfar, float* d_rdm, uint8_t* d_flag, uint8_t* d_flagV,
                        void* stream) {
    int rc = check_chain_args(ctx, "rsp_pc_mtd_cfar_dev", d_echo, dtype, batch, cfar, d_rdm, d_flag);
    if (rc) return rc;
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    return run_chain(ctx, d_echo, dtype, batch, 0, cfar, d_rdm, d_flag, d_flagV, nullptr, (hipStream_t)stream);
}

int rsp_mtd_cfar_dev(rsp_ctx* ctx, const void* d_pc, int64_t batch, const rsp_cfar_params* cfar, float* d_rdm,
                     uint8_t* d_flag, uint8_t* d_flagV, void* stream) {
    int rc = check_chain_args(ctx, "rsp_mtd_cfar_dev", d_pc, RSP_C64, batch, cfar, d_rdm, d_flag);
    if (rc) return rc;
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    return run_chain(ctx, d_pc, RSP_C64, batch, 0, cfar, d_rdm, d_flag, d_flagV, nullptr, (hipStream_t)stream, true);
}

int rsp_pc_mtd_cfar_diff_dev(rsp_ctx* ctx, const void* d_echo, int32_t dtype, int64_t batch,
                             const rsp_cfar_params* cfar, float* d_sum, float* d_diff, uint8_t* d_flag,
                             uint8_t* d_flagV, void* stream) {
    int rc = check_chain_args(ctx, "rsp_pc_mtd_cfar_diff_dev", d_echo, dtype, batch, cfar, d_sum, d_flag);
    if (rc) return rc;
    if (ctx->beams != 2)
        return fail(ctx, RSP_ERR_ARG, "rsp_pc_mtd_cfar_diff_dev: the context was created with beams=%d", ctx->beams);
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    return run_chain(ctx, d_echo, dtype, batch, 0, cfar, d_sum, d_flag, d_flagV, d_diff, (hipStream_t)stream);
}

int rsp_window_pc_mtd_cfar_dev(rsp_ctx* ctx, const void* d_frames, int32_t dtype, int64_t beams, int64_t frames,
                               int32_t win, const rsp_cfar_params* cfar, float* d_rdm, uint8_t* d_flag,
                               uint8_t* d_flagV, void* stream) {
    int rc = check_chain_args(ctx, "rsp_window_pc_mtd_cfar_dev", d_frames, dtype, frames, cfar, d_rdm, d_flag);
    if (rc) return rc;
    if (beams < 0) return fail(ctx, RSP_ERR_ARG, "rsp_window_pc_mtd_cfar_dev: beams %lld < 0", (long long)beams);
    if (ctx->beams != 1 || ctx->V != ctx->p.P)
        return fail(ctx, RSP_ERR_ARG, "rsp_window_pc_mtd_cfar_dev: needs a one-beam context with mtd_nfft = P");
    if (win < 1 || win > rsp::RSP_MAX_WIN)
        return fail(ctx, RSP_ERR_ARG, "rsp_window_pc_mtd_cfar_dev: win %d outside 1..%d", win, rsp::RSP_MAX_WIN);
    if (frames == 0 || beams == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    const int64_t P = ctx->p.P, R = ctx->p.R, Ro = ctx->p.R_out;
    const size_t esz = dtype == RSP_C64 ? 8 : 4;
    const size_t in_beam = (size_t)(frames + 1) * P * R * esz;    // bytes of one beam's frames
    const size_t out_beam = (size_t)frames * win * P * Ro;         // cells of one beam's windows
    for (int64_t b = 0; b < beams; ++b) {
        rc = run_chain(ctx, (const char*)d_frames + b * in_beam, dtype, frames, win, cfar,
                       d_rdm ? d_rdm + b * out_beam : nullptr, d_flag ? d_flag + b * out_beam : nullptr,
                       d_flagV ? d_flagV + b * out_beam : nullptr, nullptr, (hipStream_t)stream);
        if (rc) return rc;
    }
    return RSP_OK;
}

int rsp_cfar_dev(rsp_ctx* ctx, const float* d_rdm, int64_t V, int64_t R, int64_t batch,
                 const rsp_cfar_params* cfar, uint8_t* d_flag, uint8_t* d_flagV, void* stream) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_cfar_dev: null ctx");
    if (!d_rdm || !cfar || !d_flag || V < 1 || R < 1 || batch < 0)
        return fail(ctx, RSP_ERR_ARG, "rsp_cfar_dev: bad argument");
    if ((V + 1) * 4 > 64 * 1024 || R > (1 << 24))
        return fail(ctx, RSP_ERR_UNSUPPORTED, "rsp_cfar_dev: V=%lld or R=%lld too large", (long long)V, (long long)R);
    rsp::CfarVArgs cv;
    rsp::CfarRArgs cr;
    int rc = build_cfar(ctx, cfar, V, R, &cv, &cr);
    if (rc) return rc;
    if (!rsp::cfar_r_supported(cr))
        return fail(ctx, RSP_ERR_UNSUPPORTED,
                    "rsp_cfar_dev: a %lld-cell row with range window ref=%d guard=%d needs more than 160 KB of LDS "
                    "(only ref=5, guard=7 with R %% 4 == 0 is built for rows over 16320 cells)",
                    (long long)R, cr.ref, cr.save);
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    const int64_t chunk = 65535;
    if ((rc = scratch_acquire(ctx, s))) return rc;
    if (!d_flagV) {
        rc = ensure(ctx, ctx->tmp_flagV, (size_t)(batch < chunk ? batch : chunk) * V * R);
        if (rc) return rc;
    }
    for (int64_t c0 = 0; c0 < batch; c0 += chunk) {
        const int64_t n = batch - c0 < chunk ? batch - c0 : chunk;
        const float* rdm = d_rdm + (size_t)c0 * V * R;
        uint8_t* fv = d_flagV ? d_flagV + (size_t)c0 * V * R : (uint8_t*)ctx->tmp_flagV.p;
        uint8_t* fl = d_flag + (size_t)c0 * V * R;
        HIP_TRY(ctx, timed(ctx, RSP_K_CFAR_V, s, [&] { return rsp::launch_cfar_v(rdm, fv, (int)n, (int)V, (int)R, cv, s); }));
        HIP_TRY(ctx, timed(ctx, RSP_K_CFAR_R, s, [&] { return rsp::launch_cfar_r(rdm, fv, fl, (int)n, cr, s); }));
    }
    return scratch_release(ctx, s);
}

// ------------------------------------------------------------------ ordered-statistic CFAR
// rsp_os_cfar_dev's checks (no context needed: `ctx` only receives the message) and argument block.
static int build_os(rsp_ctx* ctx, const char* who, int64_t V, int64_t R, int64_t batch, const rsp_cfar_params* cfar,
                    const rsp_os_params* os, rsp::OsArgs* a) {
    if (!cfar || !os) return fail(ctx, RSP_ERR_ARG, "%s: null %s", who, !cfar ? "cfar" : "os");
    if (V < 1 || R < 1 || batch < 0)
        return fail(ctx, RSP_ERR_ARG, "%s: bad shape V = %lld, R = %lld, batch = %lld", who, (long long)V, (long long)R,
                    (long long)batch);
    if (R > (1 << 24)) return fail(ctx, RSP_ERR_UNSUPPORTED, "%s: R = %lld over 2^24 not built", who, (long long)R);
    rsp::CfarVArgs cv;
    rsp::CfarRArgs cr;
    int rc = build_cfar(ctx, cfar, V, R, &cv, &cr);
    if (rc) return rc;
    if (!std::isfinite(cfar->TV) || !(cfar->TV > 0) || !std::isfinite((float)cfar->TV))
        return fail(ctx, RSP_ERR_ARG, "%s: TV = %g must be finite and > 0", who, cfar->TV);
    if (cfar->rFlag && (!std::isfinite(cfar->TR) || !(cfar->TR > 0) || !std::isfinite((float)cfar->TR)))
        return fail(ctx, RSP_ERR_ARG, "%s: TR = %g must be finite and > 0", who, cfar->TR);
    if ((os->unionV != 0 && os->unionV != 1) || (os->unionR != 0 && os->unionR != 1))
        return fail(ctx, RSP_ERR_ARG, "%s: union flags %d, %d must be 0 or 1", who, os->unionV, os->unionR);
    if ((cfar->methodV != 0 && cfar->methodV != 1) || (cfar->rFlag && cfar->methodR != 0 && cfar->methodR != 1))
        return fail(ctx, RSP_ERR_ARG, "%s: method %d, %d must be 0 (GO) or 1 (SO)", who, cfar->methodV, cfar->methodR);
    if (cfar->refV > RSP_OS_MAX_REF || (cfar->rFlag && cfar->refR > RSP_OS_MAX_REF))
        return fail(ctx, RSP_ERR_UNSUPPORTED, "%s: ref %d / %d over %d cells per side not built", who, cfar->refV,
                    cfar->refR, RSP_OS_MAX_REF);
    if (V > RSP_OS_MAX_V)
        return fail(ctx, RSP_ERR_UNSUPPORTED, "%s: V = %lld over %d rows not built", who, (long long)V, RSP_OS_MAX_V);
    const int kmaxV = os->unionV ? 2 * cfar->refV : cfar->refV, kmaxR = os->unionR ? 2 * cfar->refR : cfar->refR;
    if (os->kV < 1 || os->kV > kmaxV)
        return fail(ctx, RSP_ERR_ARG, "%s: kV = %d outside 1..%d (%s, refV = %d)", who, os->kV, kmaxV,
                    os->unionV ? "union" : "per side", cfar->refV);
    if (cfar->rFlag && (os->kR < 1 || os->kR > kmaxR))
        return fail(ctx, RSP_ERR_ARG, "%s: kR = %d outside 1..%d (%s, refR = %d)", who, os->kR, kmaxR,
                    os->unionR ? "union" : "per side", cfar->refR);
    if (os->ld < 0 || os->cpi_stride < 0) return fail(ctx, RSP_ERR_ARG, "%s: negative row pitch / CPI stride", who);
    const int64_t ld = os->ld ? os->ld : R, cs = os->cpi_stride ? os->cpi_stride : V * ld;
    if (ld < R || cs < (V - 1) * ld + R)
        return fail(ctx, RSP_ERR_ARG, "%s: row pitch %lld / CPI stride %lld too small for %lld x %lld", who,
                    (long long)ld, (long long)cs, (long long)V, (long long)R);
    std::memset(a, 0, sizeof(*a));
    a->V = (int)V;
    a->R = (int)R;
    a->lo = cv.lo;
    a->hi = cv.hi;
    a->cz_lo = cv.cz_lo;
    a->cz_hi = cv.cz_hi;
    a->nseg = cv.nseg;
    for (int s = 0; s < cv.nseg; ++s) {
        a->seg_lo[s] = cv.seg_lo[s];
        a->seg_hi[s] = cv.seg_hi[s];
    }
    a->rflag = cr.rflag;
    a->v = rsp::OsTest{cfar->refV, cfar->saveV, os->kV, os->unionV ? rsp::kOsUnion : cfar->methodV, (float)cfar->TV};
    a->r = rsp::OsTest{cfar->refR, cfar->saveR, os->kR, os->unionR ? rsp::kOsUnion : cfar->methodR, (float)cfar->TR};
    a->ld = a->fv_ld = ld;
    a->cs = a->fv_cs = cs;
    return RSP_OK;
}

int rsp_os_cfar_dev(rsp_ctx* ctx, const float* d_rdm, int64_t V, int64_t R, int64_t batch,
                    const rsp_cfar_params* cfar, const rsp_os_params* os, uint8_t* d_flag, uint8_t* d_flagV,
                    void* stream) {
    if (!d_rdm || !d_flag) return fail(ctx, RSP_ERR_ARG, "rsp_os_cfar_dev: null %s", !d_rdm ? "d_rdm" : "d_flag");
    rsp::OsArgs a;
    int rc = build_os(ctx, "rsp_os_cfar_dev", V, R, batch, cfar, os, &a);
    if (rc) return rc;
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_os_cfar_dev: null ctx");
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    const int64_t chunk = 65535;
    const bool own_fv = a.rflag && !d_flagV;   // the Doppler flags go to the context's scratch, dense
    if (own_fv) {
        if ((rc = scratch_acquire(ctx, s))) return rc;
        if ((rc = ensure(ctx, ctx->tmp_flagV, (size_t)(batch < chunk ? batch : chunk) * V * R))) return rc;
        a.fv_ld = R;
        a.fv_cs = V * R;
    }
    for (int64_t c0 = 0; c0 < batch; c0 += chunk) {
        const int n = (int)(batch - c0 < chunk ? batch - c0 : chunk);
        const float* rdm = d_rdm + c0 * a.cs;
        uint8_t* fl = d_flag + c0 * a.cs;
        uint8_t* fv = own_fv ? (uint8_t*)ctx->tmp_flagV.p : (d_flagV ? d_flagV + c0 * a.cs : nullptr);
        HIP_TRY(ctx, timed(ctx, RSP_K_OS_V, s, [&] { return rsp::launch_os_v(rdm, a.rflag ? nullptr : fl, fv, n, a, s); }));
        if (a.rflag) HIP_TRY(ctx, timed(ctx, RSP_K_OS_R, s, [&] { return rsp::launch_os_r(rdm, fv, fl, n, a, s); }));
    }
    return own_fv ? scratch_release(ctx, s) : RSP_OK;
}

int rsp_os_cfar_plan(rsp_ctx* ctx, int64_t V, int64_t R, int64_t batch, const rsp_cfar_params* cfar,
                     const rsp_os_params* os, int32_t with_flagV, rsp_os_plan_t* out) {
    if (!out) return fail(ctx, RSP_ERR_ARG, "rsp_os_cfar_plan: null out");
    std::memset(out, 0, sizeof(*out));
    rsp::OsArgs a;
    int rc = build_os(ctx, "rsp_os_cfar_plan", V, R, batch, cfar, os, &a);
    if (rc) return rc;
    rsp::os_v_geometry(a.V, &out->v_tile_log2, &out->v_pitch);
    out->r_stage = a.rflag ? RSP_OS_R_GATHER : RSP_OS_R_NONE;
    if (a.rflag) {
        out->r_tile = rsp::kOsRTile;
        out->r_tiles = (a.R + rsp::kOsRTile - 1) / rsp::kOsRTile;
        out->r_halo = a.r.save + a.r.ref + 2;
        out->scratch_flagV = with_flagV ? 0 : 1;
    }
    return RSP_OK;
}

int rsp_cfar_plan(rsp_ctx* ctx, int64_t V, int64_t R, int64_t batch, const rsp_cfar_params* cfar, int32_t fused,
                  int32_t with_rdm, rsp_cfar_plan_t* out) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_cfar_plan: null ctx");
    if (!out || !cfar || V < 1 || R < 1 || batch < 0) return fail(ctx, RSP_ERR_ARG, "rsp_cfar_plan: bad argument");
    std::memset(out, 0, sizeof(*out));
    out->fused = fused ? 1 : 0;
    rsp::CfarRArgs cr;
    if (!fused) {   // rsp_cfar_dev's checks and launches
        if ((V + 1) * 4 > 64 * 1024 || R > (1 << 24))
            return fail(ctx, RSP_ERR_UNSUPPORTED, "rsp_cfar_plan: V=%lld or R=%lld too large", (long long)V, (long long)R);
        rsp::CfarVArgs cv;
        int rc = build_cfar(ctx, cfar, V, R, &cv, &cr);
        if (rc) return rc;
        if (!rsp::cfar_r_supported(cr))
            return fail(ctx, RSP_ERR_UNSUPPORTED, "rsp_cfar_plan: a %lld-cell row with range window ref=%d guard=%d "
                        "needs more than 160 KB of LDS", (long long)R, cr.ref, cr.save);
        out->v_tile_log2 = rsp::cfar_v_tile_log2((int)V);
        out->r_kernel = rsp::cfar_r_select(cr, &out->r_groups);
        return RSP_OK;
    }
    // the chain (run_chain_body with win == 0)
    if (ctx->cfar_only) return fail(ctx, RSP_ERR_ARG, "context was created for CFAR only (params == NULL)");
    if (V != ctx->V || R != ctx->p.R_out)
        return fail(ctx, RSP_ERR_SHAPE, "rsp_cfar_plan: %lld x %lld is not the context's %lld x %lld RDM", (long long)V,
                    (long long)R, (long long)ctx->V, (long long)ctx->p.R_out);
    rsp::MtdArgs m = ctx->mtd;
    int rc = build_cfar(ctx, cfar, V, R, &m.cv, &cr);
    if (rc) return rc;
    out->window_compiled = rsp::mtd_window_compiled(m) ? 1 : 0;
    out->bluestein = m.bnf;
    int W = 0, T = 0;
    rsp::mtd_geometry((int)V, (int)ctx->beams, &W, &T);
    out->tile_w = W;
    out->threads = T;
    out->region = W * (int32_t)V;
    if (batch == 0) return RSP_OK;   // the call returns before any launch
    ChainLayout L;
    if ((rc = chain_layout(ctx, batch, 0, true, cr, with_rdm != 0, true, &L))) return rc;
    const rsp::ChunkPlan& plan = L.plan;
    const int64_t nchunks = plan.nchunks();
    const int ns = plan.ns;
    out->region = L.reg;
    out->nchunks = (int32_t)nchunks;
    out->nlanes = ns;
    for (int l = 0; l < ns; ++l) {
        const int64_t k = l + ns * ((nchunks - 1 - l) / ns);   // the lane's last chunk
        out->lane_chunk[l] = (int32_t)plan.cap[l];
        out->lane_last[l] = (int32_t)(plan.cstart[(size_t)k + 1] - plan.cstart[(size_t)k]);
    }
    out->flag_memset = L.fm ? 1 : 0;
    if (!cr.rflag) return RSP_OK;   // RSP_RANGE_NONE, RSP_HITS_NONE
    // the largest hit-list launch: a lane's last chunk, or (grouped) lane 0's first group
    int nr = L.nreg[0];
    if (L.grouped) {
        const int64_t on0 = (nchunks + ns - 1) / ns;   // chunks on lane 0
        const int64_t g = on0 < L.rgrp ? on0 : L.rgrp;
        const int64_t k = ns * (g - 1);
        int nlast = 0, reg = 0;
        rsp::mtd_regions((int)V, (int)R, (int)(plan.cstart[(size_t)k + 1] - plan.cstart[(size_t)k]), &nlast, &reg,
                         (int)ctx->beams);
        nr = (int)(g - 1) * L.nreg[0] + nlast;
        out->range_stage = RSP_RANGE_GROUPED;
    } else if (range_per_chunk(L) || nchunks <= ns) {   // no chunk has a successor on its lane
        out->range_stage = RSP_RANGE_PER_CHUNK;
    } else {   // the MTD launch of the lane's next chunk, as run_chain_body hands it over
        m.prev_nregions = L.nreg[0];
        m.prev_region = L.reg;
        m.prev_cr = cr;
        out->range_stage = rsp::mtd_range_job57(m) ? RSP_RANGE_JOB57 : RSP_RANGE_PREV_HITS;
    }
    out->hit_kernel = rsp::cfar_hits_select(cr, nr, L.reg, &out->hit_lanes);
    return RSP_OK;
}
