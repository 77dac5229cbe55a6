// rsp_stages.cpp -- the C ABI's stage entry points around the chain (include/rsp.h): post-detection
// measurement, plot condensation, clutter map, Doppler line width, detection scoring, echo pre-filters, target
// injection, raw-data ingest, the legacy record ingest, tracking, post-detection integration and the fusion
// of stacked beams.  Each validates its arguments and launches its stage's kernels (rsp_<stage>.hip); the
// context, the presets and the PC -> MTD -> CFAR chain are in rsp_capi.cpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "rsp_ctx.h"
#include "rsp_measplan.h"

using rsp::make_window;
using rsp::scratch_acquire;
using rsp::scratch_release;
using rsp::upload;

// ------------------------------------------------------------------ post-detection measurement
// Everything rsp_motion_measure_dev checks about the shape and the parameters, for it and for
// rsp_measure_plan; fills the resolved pitches.
static int measure_check(rsp_ctx* ctx, const char* who, int64_t V, int64_t R, int64_t batch,
                         const rsp_measure_params* mp, int64_t* ld_out, int64_t* cs_out) {
    const int64_t n = 2 * (int64_t)mp->extra_dots + 1;
    if (mp->extra_dots < 1 || mp->extra_dots > 4)
        return fail(ctx, RSP_ERR_UNSUPPORTED, "%s: extra_dots %d outside 1..4", who, mp->extra_dots);
    if (mp->r_interp < 1 || mp->r_interp > 64 || mp->v_interp < 1 || mp->v_interp > 64)
        return fail(ctx, RSP_ERR_ARG, "%s: interpolation factors %d, %d outside 1..64", who, mp->r_interp,
                    mp->v_interp);
    if (V < 1 || R < 1 || V > (1 << 20) || R > (1 << 20) || V * R > (int64_t)1 << 31 || batch > 0x7fffffff)
        return fail(ctx, RSP_ERR_ARG, "%s: bad shape %lld x %lld x %lld", who, (long long)batch, (long long)V,
                    (long long)R);
    if (R < n || mp->mtd0_num < 0 || V - 2 * (int64_t)mp->mtd0_num - 1 < n)
        return fail(ctx, RSP_ERR_ARG, "%s: %lld range bins / %lld unzeroed rows are fewer than 2*extraDots+1", who,
                    (long long)R, (long long)(V - 2 * (int64_t)mp->mtd0_num - 1));
    const int64_t ld = mp->ld ? mp->ld : R, cs = mp->cpi_stride ? mp->cpi_stride : V * ld;
    if (ld < R || cs < (V - 1) * ld + R)
        return fail(ctx, RSP_ERR_ARG, "%s: row pitch %lld / CPI stride %lld too small for %lld x %lld", who,
                    (long long)ld, (long long)cs, (long long)V, (long long)R);
    *ld_out = ld;
    *cs_out = cs;
    return RSP_OK;
}

int rsp_measure_plan(rsp_ctx* ctx, const uint8_t* d_flag, int64_t V, int64_t R, int64_t batch,
                     const rsp_measure_params* mp, rsp_measure_plan_t* out) {
    if (!mp || !d_flag || !out || batch < 0) return fail(ctx, RSP_ERR_ARG, "rsp_measure_plan: bad argument");
    int64_t ld = 0, cs = 0;
    int rc = measure_check(ctx, "rsp_measure_plan", V, R, batch, mp, &ld, &cs);
    if (rc) return rc;
    const rsp::MeasPlan p = rsp::meas_plan(V, R, ld, cs, (uintptr_t)d_flag, rsp::measure_bands((int)V, (int)batch));
    memset(out, 0, sizeof(*out));
    out->wide = p.wide ? 1 : 0;
    out->cw = p.cw;
    out->groups = p.G;
    out->slices = p.S;
    out->rows = p.rows;
    out->q = p.q;
    out->passes = p.passes;
    out->bands = p.bands;
    return RSP_OK;
}

int rsp_motion_measure_dev(rsp_ctx* ctx, const float* d_sum, const float* d_diff, const uint8_t* d_flag, int64_t V,
                           int64_t R, int64_t batch, const rsp_measure_params* mp, const double* d_r_scale,
                           const double* d_v_scale, int64_t max_hits, double* d_est, int32_t* d_cells,
                           int32_t* d_count, void* stream) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_motion_measure_dev: null ctx");
    if (!mp || !d_sum || !d_diff || !d_flag || !d_r_scale || !d_v_scale || !d_count || batch < 0 || max_hits < 0 ||
        (max_hits > 0 && !d_est))
        return fail(ctx, RSP_ERR_ARG, "rsp_motion_measure_dev: bad argument");
    int64_t ld = 0, cs = 0;
    int vrc = measure_check(ctx, "rsp_motion_measure_dev", V, R, batch, mp, &ld, &cs);
    if (vrc) return vrc;
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    rsp::MeasureArgs a;
    a.ld = ld;
    a.cs = cs;
    a.extra_dots = mp->extra_dots;
    a.r_interp = mp->r_interp;
    a.v_interp = mp->v_interp;
    a.mtd0_num = mp->mtd0_num;
    a.beam_pos_num = mp->beam_pos_num;
    a.delta_r = mp->delta_r;
    a.delta_v = mp->delta_v;
    a.k_value = mp->k_value;
    a.beam_angle_step = mp->beam_angle_step;
    a.ele_comp = mp->ele_comp;
    a.ele_sys_err = mp->ele_sys_err;
    const int nb = rsp::measure_bands((int)V, (int)batch);
    int rc = scratch_acquire(ctx, (hipStream_t)stream);
    if (rc) return rc;
    if (nb > 1) {
        rc = ensure(ctx, ctx->meas_band, (size_t)batch * nb * R * sizeof(int32_t));
        if (rc != RSP_OK) return rc;
    }
    HIP_TRY(ctx, rsp::launch_measure(d_sum, d_diff, d_flag, (int)V, (int)R, (int)batch, a, d_r_scale, d_v_scale,
                                     max_hits, d_est, d_cells, d_count, (int32_t*)ctx->meas_band.p, nb,
                                     (hipStream_t)stream));
    return scratch_release(ctx, (hipStream_t)stream);
}

// ------------------------------------------------------------------ plot condensation
// Scratch budget of one chunk of CPIs: a larger batch runs as consecutive chunks on the stream.
// Chunks are kept large because the peaks' hit list costs one workgroup's scan of a whole plane
// per launch, whatever the number of CPIs in it (2048 x 512 at batch 256: 5 chunks under a 1 GiB
// budget took 3.5 ms, of which 3 ms were the five hit lists).
static constexpr size_t kCondenseChunkBytes = (size_t)8 << 30;

int rsp_condense_dev(rsp_ctx* ctx, const float* d_amp, const uint8_t* d_flag, int64_t V, int64_t R, int64_t batch,
                     const rsp_condense_params* cp, uint8_t* d_peak, int32_t max_plots, int32_t* d_plots,
                     int32_t* d_count, void* stream) {
    // everything that can be checked on the host comes before the context is looked at
    if (!cp || !d_amp || !d_flag || !d_peak || !d_count)
        return fail(ctx, RSP_ERR_ARG, "rsp_condense_dev: null argument");
    if (cp->gap_v < 0 || cp->gap_v > 4 || cp->gap_r < 0 || cp->gap_r > 4)
        return fail(ctx, RSP_ERR_ARG, "rsp_condense_dev: gap %d, %d outside 0..4", cp->gap_v, cp->gap_r);
    if ((cp->wrap_v != 0 && cp->wrap_v != 1) || cp->reserved != 0)
        return fail(ctx, RSP_ERR_ARG, "rsp_condense_dev: wrap_v %d / reserved %d", cp->wrap_v, cp->reserved);
    if (V < 1 || R < 1 || batch < 0 || batch > 0x7fffffff || max_plots < 0)
        return fail(ctx, RSP_ERR_ARG, "rsp_condense_dev: bad shape %lld x %lld x %lld, max_plots %d", (long long)batch,
                    (long long)V, (long long)R, max_plots);
    if (cp->wrap_v && V <= 2 * (int64_t)cp->gap_v)
        return fail(ctx, RSP_ERR_ARG, "rsp_condense_dev: wrap_v needs V > 2*gap_v (V = %lld, gap_v = %d)", (long long)V,
                    cp->gap_v);
    if (V > ((int64_t)1 << 31) || R > ((int64_t)1 << 31) || V * R >= (int64_t)1 << 31)
        return fail(ctx, RSP_ERR_UNSUPPORTED, "rsp_condense_dev: %lld x %lld cells (the cell index is int32)",
                    (long long)V, (long long)R);
    const int64_t ld = cp->ld ? cp->ld : R, cs = cp->cpi_stride ? cp->cpi_stride : V * ld;
    if (ld < R || cs < (V - 1) * ld + R)
        return fail(ctx, RSP_ERR_ARG, "rsp_condense_dev: row pitch %lld / CPI stride %lld too small for %lld x %lld",
                    (long long)ld, (long long)cs, (long long)V, (long long)R);
    if ((const uint8_t*)d_peak == d_flag) return fail(ctx, RSP_ERR_ARG, "rsp_condense_dev: d_peak == d_flag");
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_condense_dev: null ctx");
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    rsp::CondenseArgs a{};
    a.V = (int)V;
    a.R = (int)R;
    a.gap_v = cp->gap_v;
    a.gap_r = cp->gap_r;
    a.wrap_v = cp->wrap_v;
    a.max_plots = max_plots;
    a.ld = ld;
    a.cs = cs;
    a.cells = (size_t)V * (size_t)R;
    const size_t per = rsp::condense_scratch_per_cpi(V, R, d_plots ? max_plots : 0);
    int64_t chunk = (int64_t)(kCondenseChunkBytes / per);
    chunk = chunk < 1 ? 1 : (chunk > 32768 ? 32768 : chunk);
    if (chunk > batch) chunk = batch;
    int rc = scratch_acquire(ctx, (hipStream_t)stream);
    if (rc) return rc;
    rc = ensure(ctx, ctx->cond_tmp, (size_t)chunk * per);
    if (rc != RSP_OK) return rc;
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
        const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
        HIP_TRY(ctx, rsp::launch_condense(d_amp + b0 * cs, d_flag + b0 * cs, d_peak + b0 * cs, (int)nb, a,
                                          d_plots ? d_plots + b0 * (int64_t)max_plots * 8 : nullptr, d_count + b0 * 2,
                                          ctx->cond_tmp.p, (hipStream_t)stream));
    }
    return scratch_release(ctx, (hipStream_t)stream);
}

// ------------------------------------------------------------------ clutter map
// Everything the host can check without a context; fills the resolved shape and the plan.
static int cmap_check(rsp_ctx* ctx, const char* who, int64_t R, int64_t batch, const rsp_cmap_params* mp, rsp::CmapArgs* a,
                      int64_t* Vout) {
    if (!mp) return fail(ctx, RSP_ERR_ARG, "%s: null argument", who);
    const int64_t P = mp->P, V = mp->V ? mp->V : mp->P;
    if (P < 2 || P > ((int64_t)1 << 24) || V < P || V > ((int64_t)1 << 30))
        return fail(ctx, RSP_ERR_ARG, "%s: bad P = %lld / V = %lld (2 <= P <= V)", who, (long long)P, (long long)V);
    if (R < 1 || R > 0x7fffffff || batch < 0 || batch > 0x7fffffff)
        return fail(ctx, RSP_ERR_ARG, "%s: bad shape R = %lld, batch = %lld", who, (long long)R, (long long)batch);
    if (mp->beams != 1 && mp->beams != 2) return fail(ctx, RSP_ERR_ARG, "%s: beams = %d (1 or 2)", who, mp->beams);
    if (mp->window != RSP_WIN_KAISER && mp->window != RSP_WIN_HAMMING && mp->window != RSP_WIN_RECT)
        return fail(ctx, RSP_ERR_ARG, "%s: unknown window %d", who, mp->window);
    if (mp->window == RSP_WIN_KAISER && !(mp->window_beta >= 0.0 && mp->window_beta < 700.0))
        return fail(ctx, RSP_ERR_ARG, "%s: window_beta %g", who, mp->window_beta);
    const int64_t K = (int64_t)mp->q_hi - (int64_t)mp->q_lo + 1;
    if (K < 1 || K > RSP_CMAP_MAX_BINS)
        return fail(ctx, RSP_ERR_ARG, "%s: K = %lld bins (q %d..%d) outside 1..%d", who, (long long)K, mp->q_lo,
                    mp->q_hi, RSP_CMAP_MAX_BINS);
    const int64_t qa = std::llabs((long long)mp->q_lo), qb = std::llabs((long long)mp->q_hi);
    if (2 * (qa > qb ? qa : qb) >= V)
        return fail(ctx, RSP_ERR_ARG, "%s: bins %d..%d need |q| < V/2 (V = %lld)", who, mp->q_lo, mp->q_hi,
                    (long long)V);
    if (mp->warmup < 0 || (mp->hold != 0 && mp->hold != 1))
        return fail(ctx, RSP_ERR_ARG, "%s: warmup %d / hold %d", who, mp->warmup, mp->hold);
    if (!(mp->T > 0.0) || !std::isfinite(mp->T)) return fail(ctx, RSP_ERR_ARG, "%s: threshold T = %g", who, mp->T);
    if (!(mp->w > 0.0 && mp->w <= 1.0)) return fail(ctx, RSP_ERR_ARG, "%s: w = %g outside (0, 1]", who, mp->w);
    const int64_t ld = mp->ld ? mp->ld : R;
    if (ld < R || ld > ((int64_t)1 << 40))
        return fail(ctx, RSP_ERR_ARG, "%s: row pitch %lld too small for %lld columns", who, (long long)ld, (long long)R);
    const int64_t cs = mp->cpi_stride ? mp->cpi_stride : mp->beams * P * ld;
    if (cs < 1) return fail(ctx, RSP_ERR_ARG, "%s: CPI stride %lld", who, (long long)cs);
    a->P = (int)P;
    a->R = (int)R;
    a->K = (int)K;
    a->beams = mp->beams;
    a->warmup = mp->warmup;
    a->hold = mp->hold;
    a->T = (float)mp->T;
    a->w = (float)mp->w;
    a->ld = ld;
    a->cs = cs;
    int passes = 0;
    rsp::cmap_plan(P, R, K, ld, cs, &a->kb, &passes, &a->vec, &a->split);
    a->kpad = passes * a->kb;
    *Vout = V;
    return RSP_OK;
}

int rsp_cmap_plan(rsp_ctx* ctx, int64_t R, int64_t batch, const rsp_cmap_params* mp, rsp_cmap_plan_t* out) {
    if (!out) return fail(ctx, RSP_ERR_ARG, "rsp_cmap_plan: null argument");
    rsp::CmapArgs a{};
    int64_t V = 0;
    int rc = cmap_check(ctx, "rsp_cmap_plan", R, batch, mp, &a, &V);
    if (rc) return rc;
    memset(out, 0, sizeof(*out));
    out->K = a.K;
    out->kpad = a.kpad;
    out->bins_per_pass = a.kb;
    out->passes = a.kpad / a.kb;
    out->vec = a.vec;
    out->split = a.split;
    out->threads = 64 * a.split;
    out->table_bytes = (int64_t)a.P * a.kpad * 8;
    out->pool_bytes = batch * a.K * R * 4;
    return RSP_OK;
}

// tab[p][k] = win[p] * exp(-2 pi j (q_lo + k) p / V) for k < K, zero for the padding, fp64 -> fp32
static int cmap_table(rsp_ctx* ctx, const rsp_cmap_params* mp, const rsp::CmapArgs& a, int64_t V, const float2** out) {
    int64_t beta_bits = 0;
    if (mp->window == RSP_WIN_KAISER) memcpy(&beta_bits, &mp->window_beta, sizeof(beta_bits));
    const std::vector<int64_t> key{a.P, V, mp->window, beta_bits, mp->q_lo, mp->q_hi, a.kpad};
    auto it = ctx->cmap_tab.find(key);
    if (it != ctx->cmap_tab.end()) {
        *out = it->second;
        return RSP_OK;
    }
    const std::vector<double> win = make_window(mp->window, mp->window_beta, a.P);
    std::vector<float2> h((size_t)a.P * a.kpad, make_float2(0.0f, 0.0f));
    for (int64_t p = 0; p < a.P; ++p)
        for (int k = 0; k < a.K; ++k) {
            int64_t e = ((int64_t)(mp->q_lo + k) * p) % V;   // the angle's index, reduced in integers
            if (e < 0) e += V;
            const double ang = -2.0 * M_PI * (double)e / (double)V;
            h[(size_t)p * a.kpad + k] = make_float2((float)(win[p] * std::cos(ang)), (float)(win[p] * std::sin(ang)));
        }
    float2* d = nullptr;
    int rc = upload(ctx, h, &d);
    if (rc) return rc;
    ctx->cmap_tab[key] = d;
    *out = d;
    return RSP_OK;
}

int rsp_cmap_dev(rsp_ctx* ctx, const void* d_pc, int64_t R, int64_t batch, const rsp_cmap_params* mp,
                 const int32_t* d_slot, int32_t slots, float* d_map, int32_t* d_age, float* d_band, uint8_t* d_flag,
                 void* stream) {
    // everything that can be checked on the host comes before the context is looked at
    if (!mp || !d_pc || !d_map || !d_age || !d_flag) return fail(ctx, RSP_ERR_ARG, "rsp_cmap_dev: null argument");
    rsp::CmapArgs a{};
    int64_t V = 0;
    int rc = cmap_check(ctx, "rsp_cmap_dev", R, batch, mp, &a, &V);
    if (rc) return rc;
    if (slots < 1 || slots > 65535) return fail(ctx, RSP_ERR_ARG, "rsp_cmap_dev: slots = %d outside 1..65535", slots);
    a.slots = slots;
    if ((int64_t)a.K * R > ((int64_t)1 << 36))
        return fail(ctx, RSP_ERR_UNSUPPORTED, "rsp_cmap_dev: %d x %lld map cells per slot", a.K, (long long)R);
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_cmap_dev: null ctx");
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    const float2* tab = nullptr;
    if ((rc = cmap_table(ctx, mp, a, V, &tab))) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* band = d_band;
    if (!band) {
        if ((rc = scratch_acquire(ctx, st))) return rc;
        if ((rc = ensure(ctx, ctx->cmap_band, (size_t)batch * a.K * (size_t)R * 4)) != RSP_OK) return rc;
        band = (float*)ctx->cmap_band.p;
    }
    const float2* pc = (const float2*)d_pc;
    const int64_t cells = (int64_t)a.K * R;
    for (int64_t b0 = 0; b0 < batch; b0 += 65535) {   // gridDim.z; the bytes do not depend on the cut
        const int nb = (int)(batch - b0 < 65535 ? batch - b0 : 65535);
        // the vector width is chosen once for the call: every launch sees the same alignment
        rsp::CmapArgs ab = a;
        if (((uintptr_t)pc & 15) || ((uintptr_t)band & 7)) ab.vec = 1;
        HIP_TRY(ctx, rsp::launch_cmap_band(pc + b0 * a.cs, tab, ab, nb, band + b0 * cells, st));
    }
    HIP_TRY(ctx, rsp::launch_cmap_update(band, d_slot, a, batch, d_map, d_age, d_flag, st));
    return d_band ? RSP_OK : scratch_release(ctx, st);
}

// ------------------------------------------------------------------ Doppler line width
int rsp_spec_width_dev(rsp_ctx* ctx, const float* d_amp, const uint8_t* d_flag, int64_t V, int64_t R, int64_t batch,
                       const rsp_width_params* wp, int32_t* d_span, int32_t* d_count, void* stream) {
    // everything that can be checked on the host comes before the context is looked at
    if (!wp || !d_amp || !d_span || !d_count) return fail(ctx, RSP_ERR_ARG, "rsp_spec_width_dev: null argument");
    if (!(wp->amp_constr >= -200.0 && wp->amp_constr < 0.0))
        return fail(ctx, RSP_ERR_ARG, "rsp_spec_width_dev: amp_constr %g dB outside [-200, 0)", wp->amp_constr);
    if (wp->interp < 1 || wp->interp > 64)
        return fail(ctx, RSP_ERR_ARG, "rsp_spec_width_dev: interp %d outside 1..64", wp->interp);
    if (wp->shift != 0 && wp->shift != 1) return fail(ctx, RSP_ERR_ARG, "rsp_spec_width_dev: shift %d", wp->shift);
    if (V < RSP_WIDTH_MIN_V || V > RSP_WIDTH_MAX_V)
        return fail(ctx, RSP_ERR_ARG, "rsp_spec_width_dev: V = %lld outside %d..%d", (long long)V, RSP_WIDTH_MIN_V,
                    RSP_WIDTH_MAX_V);
    if (R < 1 || R > (1 << 24) || batch < 0 || batch > 0x7fffffff)
        return fail(ctx, RSP_ERR_ARG, "rsp_spec_width_dev: bad shape R = %lld, batch = %lld", (long long)R,
                    (long long)batch);
    if (wp->ld < 0 || wp->cpi_stride < 0)
        return fail(ctx, RSP_ERR_ARG, "rsp_spec_width_dev: negative row pitch / CPI stride");
    const int64_t ld = wp->ld ? wp->ld : R, cs = wp->cpi_stride ? wp->cpi_stride : V * ld;
    if (ld < R || ld > ((int64_t)1 << 40) || cs < (V - 1) * ld + R)
        return fail(ctx, RSP_ERR_ARG, "rsp_spec_width_dev: row pitch %lld / CPI stride %lld too small for %lld x %lld",
                    (long long)ld, (long long)cs, (long long)V, (long long)R);
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_spec_width_dev: null ctx");
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    rsp::WidthArgs a{};
    a.V = (int)V;
    a.R = (int)R;
    a.interp = wp->interp;
    a.shift = wp->shift;
    a.level = std::pow(10.0, wp->amp_constr / 20.0);
    a.ld = ld;
    a.cs = cs;
    for (int64_t b0 = 0; b0 < batch; b0 += 65535) {   // gridDim.y; a column's bytes do not depend on the cut
        const int nb = (int)(batch - b0 < 65535 ? batch - b0 : 65535);
        HIP_TRY(ctx, rsp::launch_width(d_amp + b0 * cs, d_flag ? d_flag + b0 * cs : nullptr, nb, a, d_span + b0 * R * 2,
                                       d_count + b0, (hipStream_t)stream));
    }
    return RSP_OK;
}

// ------------------------------------------------------------------ detection scoring
static const char* score_params_bad(const rsp_score_params* sp) {
    constexpr int32_t kMax = 1 << 24;
    if (sp->hv < 0 || sp->hr < 0 || sp->n_cell < 0 || sp->hv > kMax || sp->hr > kMax || sp->n_cell > kMax)
        return "box half sizes outside 0..2^24";
    if (sp->v_lim < 0 || sp->r_lim < 0) return "negative v_lim / r_lim";
    if (sp->ld < 0 || sp->cpi_stride < 0) return "negative pitch";
    return nullptr;
}

int rsp_score_dev(rsp_ctx* ctx, const uint8_t* d_flag, const float* d_rdm, int64_t V, int64_t R, int64_t batch,
                  const rsp_score_params* sp, const int32_t* d_truth, int32_t* d_rec, void* stream) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_score_dev: null ctx");
    if (!sp || !d_flag || !d_truth || !d_rec || batch < 0) return fail(ctx, RSP_ERR_ARG, "rsp_score_dev: bad argument");
    if (const char* why = score_params_bad(sp)) return fail(ctx, RSP_ERR_ARG, "rsp_score_dev: %s", why);
    // V * R below 2^31: the flag total and the packed peak index r*V + v are int32
    if (V < 1 || R < 1 || V > (1 << 20) || R > (1 << 20) || V * R >= (int64_t)1 << 31 || batch > 0x7fffffff)
        return fail(ctx, RSP_ERR_ARG, "rsp_score_dev: bad shape %lld x %lld x %lld", (long long)batch, (long long)V,
                    (long long)R);
    const int64_t ld = sp->ld ? sp->ld : R, cs = sp->cpi_stride ? sp->cpi_stride : V * ld;
    if (ld < R || cs < (V - 1) * ld + R)
        return fail(ctx, RSP_ERR_ARG, "rsp_score_dev: row pitch %lld / CPI stride %lld too small for %lld x %lld",
                    (long long)ld, (long long)cs, (long long)V, (long long)R);
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    rsp::ScoreArgs a;
    a.V = (int)V;
    a.R = (int)R;
    a.hv = sp->hv;
    a.hr = sp->hr;
    a.n_cell = sp->n_cell;
    a.v_lim = sp->v_lim;
    a.r_lim = sp->r_lim;
    a.ld = ld;
    a.cs = cs;
    HIP_TRY(ctx, rsp::launch_score(d_flag, d_rdm, d_truth, d_rec, (int)batch, a, (hipStream_t)stream));
    return RSP_OK;
}

// main_cfar.m:163-279 from the records, in the reference's operation order (host only).
int rsp_score_summary(const int32_t* rec, const int32_t* truth, int64_t batch, int64_t V, int64_t R,
                      const rsp_score_params* sp, double* fa, rsp_score_result* out) {
    if (!rec || !truth || !sp || !out || batch < 0 || V < 1 || R < 1)
        return fail(nullptr, RSP_ERR_ARG, "rsp_score_summary: bad argument");
    if (const char* why = score_params_bad(sp)) return fail(nullptr, RSP_ERR_ARG, "rsp_score_summary: %s", why);
    rsp_score_result r{};
    const double cells = (double)V * (double)R;                       // m*n (:164)
    const double dv_base = 1.0 / 0.2719, dr_base = 30.0 / 6.0;        // :237
    const double l_base = dv_base * dv_base + dr_base * dr_base;      // :266
    double d11 = 0, d01 = 0;   // fun_drate's n_p_1_1, n_p_0_1
    double a11 = 0, a00 = 0;   // fun_accuracy's n_p_1_1, n_p_0_0
    double pof_sum = 0;
    for (int64_t i = 0; i < batch; ++i) {
        const int32_t* c = rec + i * 8;
        const int32_t* t = truth + i * 3;
        const bool valid = t[2] != 0;
        const bool low = c[2] & 1, high = c[2] & 2;
        if (!valid) {
            if (fa) fa[i] = (double)c[0] / cells;                    // :171-174
            if (c[0] > 0) a00 += 1;                                  // :224-227
            continue;
        }
        ++r.n_valid;
        if (low) {   // an index below 1: the assignment at :167 stops too
            ++r.n_index_error[RSP_SCORE_FA];
            if (fa) fa[i] = NAN;
        } else if (fa) {
            fa[i] = (double)(c[0] - c[1]) / cells;                   // :167-169, :174
        }
        if (low || high) {   // the reads at :188 / :219 stop on either side
            ++r.n_index_error[RSP_SCORE_DRATE];
            ++r.n_index_error[RSP_SCORE_ACC];
        } else {
            if (c[1] > 0) {
                d11 += 1;
                a11 += 1;
            } else {
                d01 += 1;
            }
        }
        if (c[4] & 1) {
            ++r.n_index_error[RSP_SCORE_PCF];
        } else if (c[3] > 0 && c[5] > 0) {
            if (c[5] > 1) {
                ++r.n_multi_peak;
            } else {
                const double dv = std::fabs((double)t[0] - (double)c[6]), dr = std::fabs((double)t[1] - (double)c[7]);
                const double l = dv * dv + dr * dr;                  // :265
                pof_sum += l < l_base ? 1.0 - l / l_base : std::exp(1.0 - l / l_base) - 1.0;   // :267-271
                ++r.n_scored;
            }
        }
    }
    r.drate = d11 / (d11 + d01);                                     // :205 (0/0 = NaN)
    r.acc = batch ? (a11 + a00) / (double)batch : NAN;               // :232
    r.pof = pof_sum / (double)r.n_scored;                            // :278 (0/0 = NaN)
    *out = r;
    return RSP_OK;
}

// ------------------------------------------------------------------ echo pre-filters
int rsp_prefilter_dev(rsp_ctx* ctx, const void* d_in, void* d_out, int64_t P, int64_t R, int64_t batch,
                      const float* d_gain, int32_t mti_lag, void* stream) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_prefilter_dev: null ctx");
    if (!d_in || !d_out || P < 1 || R < 2 || batch < 0 || mti_lag < 0)
        return fail(ctx, RSP_ERR_ARG, "rsp_prefilter_dev: bad argument");
    if (R % 2 != 0 || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 15))
        return fail(ctx, RSP_ERR_UNSUPPORTED, "rsp_prefilter_dev: needs an even R and 16-byte aligned buffers");
    if (P > (1 << 24) || R > (1 << 24))
        return fail(ctx, RSP_ERR_ARG, "rsp_prefilter_dev: bad shape %lld x %lld", (long long)P, (long long)R);
    if (mti_lag > 0 && d_in == d_out)
        return fail(ctx, RSP_ERR_ARG, "rsp_prefilter_dev: MTI cannot run in place");
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(ctx, rsp::launch_prefilter((const float2*)d_in, (float2*)d_out, d_gain, (int)P, (int)R, batch, mti_lag,
                                       (hipStream_t)stream));
    return RSP_OK;
}

// ------------------------------------------------------------------ target injection at a set SCR
static bool ranges_overlap(const void* a, int64_t an, const void* b, int64_t bn) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bn && b0 < a0 + (uintptr_t)an;
}

// Everything rsp_scr_dev / rsp_inject_dev can check on the host, before the context is looked at
// (so a malformed call is told apart without a GPU); fills the shared part of the kernel's arguments.
static int scr_check(rsp_ctx* ctx, const char* fn, const void* d_simu, bool point, const void* d_clutter, void* d_out,
                     int64_t P, int64_t R, int64_t batch, const double* d_scr_db, const rsp_scr_params* sp,
                     rsp::InjectArgs* a, bool* vec16) {
    if (!sp || !d_clutter || !d_out || !d_scr_db || (!point && !d_simu))
        return fail(ctx, RSP_ERR_ARG, "%s: null argument", fn);
    if (P < 1 || R < 1 || batch < 0 || P > (1 << 24) || R > (1 << 24) || batch > 0x7fffffff ||
        batch * P > ((int64_t)1 << 40))
        return fail(ctx, RSP_ERR_ARG, "%s: bad shape %lld x %lld x %lld", fn, (long long)batch, (long long)P,
                    (long long)R);
    if (sp->nseg < 0 || sp->nseg > RSP_MAX_SEG)
        return fail(ctx, RSP_ERR_ARG, "%s: nseg %d outside 0..%d", fn, sp->nseg, RSP_MAX_SEG);
    if ((sp->power != RSP_SCR_ABS2 && sp->power != RSP_SCR_AS_WRITTEN) || (sp->add_clutter != 0 && sp->add_clutter != 1) ||
        sp->reserved != 0)
        return fail(ctx, RSP_ERR_ARG, "%s: power %d / add_clutter %d / reserved %d", fn, sp->power, sp->add_clutter,
                    sp->reserved);
    for (int s = 0; s < sp->nseg; ++s) {
        if (sp->seg_start[s] < 0 || sp->seg_len[s] < 1 || sp->seg_start[s] > R || sp->seg_len[s] > R - sp->seg_start[s])
            return fail(ctx, RSP_ERR_ARG, "%s: segment %d = [%lld, +%lld) is not inside [0, %lld)", fn, s,
                        (long long)sp->seg_start[s], (long long)sp->seg_len[s], (long long)R);
        if (!std::isfinite(sp->seg_db[s])) return fail(ctx, RSP_ERR_ARG, "%s: seg_db[%d] is not finite", fn, s);
        for (int q = 0; q < s; ++q)
            if (sp->seg_start[s] < sp->seg_start[q] + sp->seg_len[q] && sp->seg_start[q] < sp->seg_start[s] + sp->seg_len[s])
                return fail(ctx, RSP_ERR_ARG, "%s: segments %d and %d overlap", fn, q, s);
    }
    const int64_t ld = sp->clutter_ld ? sp->clutter_ld : R, K = sp->clutter_batch ? sp->clutter_batch : batch;
    if (ld < R) return fail(ctx, RSP_ERR_ARG, "%s: clutter_ld %lld below R = %lld", fn, (long long)ld, (long long)R);
    if (batch > 0 && (K < 1 || K > batch))
        return fail(ctx, RSP_ERR_ARG, "%s: clutter_batch %lld outside 1..%lld", fn, (long long)K, (long long)batch);
    const int64_t out_bytes = batch * P * R * 8, clut_bytes = ((K * P - 1) * ld + R) * 8;
    if (batch > 0) {
        if (d_out == d_clutter) {
            if (K != batch || ld != R)
                return fail(ctx, RSP_ERR_ARG, "%s: d_out == d_clutter needs clutter_batch == batch and clutter_ld == R", fn);
        } else if (ranges_overlap(d_out, out_bytes, d_clutter, clut_bytes)) {
            return fail(ctx, RSP_ERR_ARG, "%s: d_out overlaps d_clutter", fn);
        }
        if (!point && d_out != d_simu && ranges_overlap(d_out, out_bytes, d_simu, out_bytes))
            return fail(ctx, RSP_ERR_ARG, "%s: d_out overlaps d_simu", fn);
    }
    if (((uintptr_t)d_out | (uintptr_t)d_clutter | (uintptr_t)d_simu) & 7)
        return fail(ctx, RSP_ERR_ARG, "%s: buffers must be 8-byte aligned", fn);
    *a = rsp::InjectArgs{};
    a->P = (int)P;
    a->R = (int)R;
    a->nseg = sp->nseg;
    a->power = sp->power;
    a->add = sp->add_clutter;
    for (int s = 0; s < sp->nseg; ++s) {
        a->lo[s] = (int)sp->seg_start[s];
        a->hi[s] = (int)(sp->seg_start[s] + sp->seg_len[s]);
        a->db[s] = sp->seg_db[s];
    }
    a->c_ld = ld;
    a->c_cs = P * ld;
    a->c_batch = (int)(K > 0 ? K : 1);
    a->simu = (const float2*)d_simu;
    a->clutter = (const float2*)d_clutter;
    a->out = (float2*)d_out;
    a->scr_db = d_scr_db;
    *vec16 = R % 2 == 0 && ld % 2 == 0 && !(((uintptr_t)d_out | (uintptr_t)d_clutter | (uintptr_t)d_simu) & 15);
    return RSP_OK;
}

static int scr_run(rsp_ctx* ctx, rsp::InjectArgs& a, int64_t batch, bool vec16, hipStream_t s) {
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    int rc = scratch_acquire(ctx, s);
    if (rc) return rc;
    rc = ensure(ctx, ctx->scr_ps, (size_t)batch * (size_t)rsp::inject_ps_stride(a.P) * sizeof(double));
    if (rc) return rc;
    a.ps = (double*)ctx->scr_ps.p;
    HIP_TRY(ctx, rsp::launch_inject(a, batch, vec16, s));
    return scratch_release(ctx, s);
}

int rsp_scr_dev(rsp_ctx* ctx, const void* d_simu, const void* d_clutter, void* d_out, int64_t P, int64_t R,
                int64_t batch, const double* d_scr_db, const rsp_scr_params* sp, void* stream) {
    rsp::InjectArgs a;
    bool vec16 = false;
    const int rc = scr_check(ctx, "rsp_scr_dev", d_simu, false, d_clutter, d_out, P, R, batch, d_scr_db, sp, &a, &vec16);
    if (rc) return rc;
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_scr_dev: null ctx");
    return scr_run(ctx, a, batch, vec16, (hipStream_t)stream);
}

int rsp_inject_dev(rsp_ctx* ctx, const void* d_clutter, void* d_out, int64_t P, int64_t R, int64_t batch,
                   const void* d_wf, const int64_t* wf_off, const int32_t* d_delay, const double* d_dphi,
                   const double* d_scr_db, const rsp_scr_params* sp, void* stream) {
    rsp::InjectArgs a;
    bool vec16 = false;
    if (!d_wf || !wf_off || !d_delay || !d_dphi) return fail(ctx, RSP_ERR_ARG, "rsp_inject_dev: null argument");
    const int rc = scr_check(ctx, "rsp_inject_dev", nullptr, true, d_clutter, d_out, P, R, batch, d_scr_db, sp, &a, &vec16);
    if (rc) return rc;
    if (((uintptr_t)d_wf & 7) || ((uintptr_t)d_delay & 3) || ((uintptr_t)d_dphi & 7))
        return fail(ctx, RSP_ERR_ARG, "rsp_inject_dev: misaligned argument");
    for (int s = 0; s <= sp->nseg; ++s) {
        if (wf_off[s] < 0 || wf_off[s] > 0x7fffffff || (s > 0 && wf_off[s] < wf_off[s - 1]))
            return fail(ctx, RSP_ERR_ARG, "rsp_inject_dev: wf_off[%d] = %lld (offsets must not decrease)", s,
                        (long long)wf_off[s]);
        a.wf_off[s] = (int)wf_off[s];
    }
    for (int s = sp->nseg + 1; s <= RSP_MAX_SEG; ++s) a.wf_off[s] = a.wf_off[sp->nseg];
    a.wf = (const float2*)d_wf;
    a.delay = d_delay;
    a.dphi = d_dphi;
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "rsp_inject_dev: null ctx");
    return scr_run(ctx, a, batch, vec16, (hipStream_t)stream);
}

int rsp_scr_gain(int32_t power, const double sum_simu[2], const double sum_clutter[2], int64_t n, double scr_db,
                 double gain[2]) {
    if (!sum_simu || !sum_clutter || !gain || n < 1 || (power != RSP_SCR_ABS2 && power != RSP_SCR_AS_WRITTEN))
        return fail(nullptr, RSP_ERR_ARG, "rsp_scr_gain: bad argument");
    rsp::scr_gain(power, sum_simu[0], sum_simu[1], sum_clutter[0], sum_clutter[1], (double)n, rsp::scr_lin(scr_db), &gain[0],
                  &gain[1]);
    return RSP_OK;
}

// ------------------------------------------------------------------ raw-data ingest
static int ingest_shape(rsp_ctx* ctx, const rsp_ingest_params* p, int64_t* rec) {
    if (!p) return fail(ctx, RSP_ERR_ARG, "ingest: null params");
    if (p->prt_num < 0 || p->point_prt <= 0 || p->channel_num <= 0 || p->channel_num > 255 || p->beam_num <= 0 ||
        p->bytes_head < 64 || p->bytes_realtime < 0 || p->bytes_tail < 0 || p->bytes_head % 4 || p->bytes_realtime % 4)
        return fail(ctx, RSP_ERR_ARG, "ingest: bad shape (prt %d, point %d, channels %d, beams %d, head %d)",
                    p->prt_num, p->point_prt, p->channel_num, p->beam_num, p->bytes_head);
    // FrameDataRead_xzr.m:108-119: DDC payload = samples * channels * 2 (I, Q) * 2 bytes, padded to 64 B
    int64_t sig = (int64_t)p->point_prt * p->channel_num * 4;
    if (sig % 64) sig += 64 - sig % 64;
    if (sig >= 0x80000000ll) return fail(ctx, RSP_ERR_UNSUPPORTED, "ingest: payload of %lld bytes", (long long)sig);
    *rec = (int64_t)p->bytes_head + p->bytes_realtime + sig + p->bytes_tail;
    return RSP_OK;
}

int rsp_ingest_record_bytes(const rsp_ingest_params* p, int64_t* bytes) {
    if (!bytes) return fail(nullptr, RSP_ERR_ARG, "rsp_ingest_record_bytes: null output");
    return ingest_shape(nullptr, p, bytes);
}

static int ingest_run(rsp_ctx* ctx, const char* who, bool ddc_only, const uint8_t* d_stream, int64_t nbytes,
                      const rsp_ingest_params* p, const float* d_dbf, void* d_out, int64_t beam_stride,
                      uint16_t* d_servo, int32_t* d_status, void* stream) {
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "%s: null ctx", who);
    int64_t rec = 0;
    int rc = ingest_shape(ctx, p, &rec);
    if (rc) return rc;
    if (!d_stream || nbytes < 0 || !d_dbf || !d_out || !d_status)
        return fail(ctx, RSP_ERR_ARG, "%s: null buffer or negative byte count", who);
    const int64_t plane = (int64_t)p->prt_num * p->point_prt;
    if (beam_stride == 0) beam_stride = plane;
    if (beam_stride < plane) return fail(ctx, RSP_ERR_ARG, "%s: beam_stride %lld < prt*point %lld", who,
                                         (long long)beam_stride, (long long)plane);
    if (p->prt_num == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    // per-PRT record offsets and types, written by the check kernel for the decode kernel
    // (stream-ordered on the caller's stream; one frame at a time per context)
    rc = ensure(ctx, ctx->ing_meta, (size_t)p->prt_num * (sizeof(int64_t) + sizeof(int32_t)));
    if (rc) return rc;
    rsp::IngestArgs a{};
    a.ddc_only = ddc_only ? 1 : 0;
    a.offs = (int64_t*)ctx->ing_meta.p;
    a.types = (int32_t*)((int64_t*)ctx->ing_meta.p + p->prt_num);
    a.prt_num = p->prt_num;
    a.point_prt = p->point_prt;
    a.channel_num = p->channel_num;
    a.beam_num = p->beam_num;
    a.bytes_head = p->bytes_head;
    a.bytes_realtime = p->bytes_realtime;
    a.bytes_tail = p->bytes_tail;
    a.rec_bytes = rec;
    a.beam_stride = beam_stride;
    HIP_TRY(ctx, rsp::launch_ingest(d_stream, nbytes, a, (const float2*)d_dbf, (float2*)d_out, d_servo, d_status,
                                    (hipStream_t)stream));
    return RSP_OK;
}

int rsp_ingest_ddc_dev(rsp_ctx* ctx, const uint8_t* d_stream, int64_t nbytes, const rsp_ingest_params* p,
                       const float* d_dbf, void* d_out, int64_t beam_stride, uint16_t* d_servo,
                       int32_t* d_status, void* stream) {
    return ingest_run(ctx, "rsp_ingest_ddc_dev", true, d_stream, nbytes, p, d_dbf, d_out, beam_stride, d_servo,
                      d_status, stream);
}

int rsp_ingest_frame_dev(rsp_ctx* ctx, const uint8_t* d_stream, int64_t nbytes, const rsp_ingest_params* p,
                         const float* d_dbf, void* d_out, int64_t beam_stride, uint16_t* d_servo,
                         int32_t* d_status, void* stream) {
    return ingest_run(ctx, "rsp_ingest_frame_dev", false, d_stream, nbytes, p, d_dbf, d_out, beam_stride, d_servo,
                      d_status, stream);
}

// ------------------------------------------------------------------ legacy two-beam 24-bit records
static int legacy_shape(const char* who, const rsp_legacy_ingest_params* p, int64_t* rec) {
    if (!p) return fail(nullptr, RSP_ERR_ARG, "%s: null params", who);
    // a grid dimension per PRT and per frame; rows * rec_bytes stays far inside int64
    if (p->prt_num < 1 || p->prt_num > 65535 || p->point_prt < 1 || p->point_prt > (1 << 24) || p->nframes < 1 ||
        p->nframes > 65535 || p->reserved != 0 || (int64_t)p->prt_num * p->nframes > 0x7fffffff)
        return fail(nullptr, RSP_ERR_ARG, "%s: bad shape (prt %d, point %d, frames %d, reserved %d)", who, p->prt_num,
                    p->point_prt, p->nframes, p->reserved);
    *rec = rsp::legacy_record_bytes(p->point_prt);
    return RSP_OK;
}

int rsp_legacy_record_bytes(const rsp_legacy_ingest_params* p, int64_t* bytes) {
    if (!bytes) return fail(nullptr, RSP_ERR_ARG, "rsp_legacy_record_bytes: null output");
    return legacy_shape("rsp_legacy_record_bytes", p, bytes);
}

int rsp_ingest_legacy_dev(rsp_ctx* ctx, const uint8_t* d_stream, int64_t nbytes, const rsp_legacy_ingest_params* p,
                          void* d_out, int64_t beam_stride, int64_t frame_stride, double* d_angle, int32_t* d_head,
                          int32_t* d_status, void* stream) {
    // everything is checked before the context is looked at (a malformed call is told apart without a GPU)
    const char* who = "rsp_ingest_legacy_dev";
    int64_t rec = 0;
    const int rc = legacy_shape(who, p, &rec);
    if (rc) return rc;
    if (!d_stream || !d_out || !d_status) return fail(nullptr, RSP_ERR_ARG, "%s: null argument", who);
    if (nbytes < 0) return fail(nullptr, RSP_ERR_ARG, "%s: negative byte count %lld", who, (long long)nbytes);
    const int64_t plane = (int64_t)p->prt_num * p->point_prt, nf = p->nframes;
    if (beam_stride == 0) beam_stride = plane;
    if (frame_stride == 0) frame_stride = 2 * beam_stride;
    // the 2 * nframes planes must not overlap: frames of [left, right] pairs, or two stacks of frames
    const bool in_range = beam_stride > 0 && frame_stride > 0 && beam_stride <= ((int64_t)1 << 40) &&
                          frame_stride <= ((int64_t)1 << 40);
    const bool frame_major = in_range && beam_stride >= plane && (nf == 1 || frame_stride >= beam_stride + plane);
    const bool beam_major = in_range && frame_stride >= plane && beam_stride >= (nf - 1) * frame_stride + plane;
    if (!(frame_major || beam_major))
        return fail(nullptr, RSP_ERR_ARG, "%s: planes of %lld elements overlap with beam_stride %lld, frame_stride %lld", who,
                    (long long)plane, (long long)beam_stride, (long long)frame_stride);
    // the payload is read as dwords (the record size is a multiple of 4); float2 / double stores
    if ((uintptr_t)d_stream & 3) return fail(nullptr, RSP_ERR_ARG, "%s: d_stream must be 4-byte aligned", who);
    if (((uintptr_t)d_out & 7) || ((uintptr_t)d_angle & 7) || ((uintptr_t)d_head & 3) || ((uintptr_t)d_status & 3))
        return fail(nullptr, RSP_ERR_ARG, "%s: misaligned output (d_out, d_angle: 8 bytes; d_head, d_status: 4)", who);
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "%s: null ctx", who);
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    rsp::LegacyIngestArgs a{};
    a.prt_num = p->prt_num;
    a.point_prt = p->point_prt;
    a.nframes = p->nframes;
    a.rows = (int64_t)p->prt_num * nf;
    a.rec_bytes = rec;
    a.nbytes = nbytes;
    a.rows_decoded = rsp::legacy_rows_decoded(nbytes, rec, a.rows);
    a.beam_stride = beam_stride;
    a.frame_stride = frame_stride;
    HIP_TRY(ctx, rsp::launch_ingest_legacy(d_stream, a, (float2*)d_out, d_angle, d_head, d_status, (hipStream_t)stream));
    return RSP_OK;
}

// ------------------------------------------------------------------ tracking
int rsp_track_dev(rsp_ctx* ctx, const double* d_est, const int32_t* d_count, int64_t max_hits, int64_t batch,
                  const rsp_track_params* tp, const int32_t* d_slot, const double* d_dt, int32_t slots, double* d_state_f,
                  int32_t* d_state_i, int32_t* d_meta, int32_t* d_assign, double* d_snap_f, int32_t* d_snap_i,
                  int32_t* d_tcount, void* stream) {
    // everything that can be checked on the host comes before the context is looked at
    const char* who = "rsp_track_dev";
    if (!tp || !d_count || !d_state_f || !d_state_i || !d_meta || !d_tcount)
        return fail(ctx, RSP_ERR_ARG, "%s: null argument", who);
    if (max_hits < 0 || max_hits > 0x7fffffff / 3 || batch < 0 || batch > 0x7fffffff)
        return fail(ctx, RSP_ERR_ARG, "%s: bad shape max_hits = %lld, batch = %lld", who, (long long)max_hits,
                    (long long)batch);
    if (max_hits > 0 && (!d_est || !d_assign)) return fail(ctx, RSP_ERR_ARG, "%s: null argument", who);
    if ((d_snap_f == nullptr) != (d_snap_i == nullptr))
        return fail(ctx, RSP_ERR_ARG, "%s: d_snap_f and d_snap_i go together", who);
    if (tp->max_tracks < 1 || tp->max_tracks > RSP_TRACK_MAX_TRACKS)
        return fail(ctx, RSP_ERR_ARG, "%s: max_tracks = %d outside 1..%d", who, tp->max_tracks, RSP_TRACK_MAX_TRACKS);
    if (tp->confirm_m < 1 || tp->confirm_m > tp->confirm_n || tp->confirm_n > 32)
        return fail(ctx, RSP_ERR_ARG, "%s: confirm %d of %d (1 <= M <= N <= 32)", who, tp->confirm_m, tp->confirm_n);
    if (tp->drop_tentative < 1 || tp->drop_confirmed < 1)
        return fail(ctx, RSP_ERR_ARG, "%s: drop counts %d, %d below 1", who, tp->drop_tentative, tp->drop_confirmed);
    if (tp->reserved != 0) return fail(ctx, RSP_ERR_ARG, "%s: reserved = %d", who, tp->reserved);
    if (!(tp->dt > 0.0) || !std::isfinite(tp->dt)) return fail(ctx, RSP_ERR_ARG, "%s: dt = %g", who, tp->dt);
    if (tp->rate_sign != 1.0 && tp->rate_sign != -1.0)
        return fail(ctx, RSP_ERR_ARG, "%s: rate_sign = %g (+1 or -1)", who, tp->rate_sign);
    if (!(tp->gate_r > 0.0) || !std::isfinite(tp->gate_r) || !(tp->gate_v > 0.0) || !std::isfinite(tp->gate_v))
        return fail(ctx, RSP_ERR_ARG, "%s: gate %g, %g", who, tp->gate_r, tp->gate_v);
    if (!(tp->alpha_r > 0.0 && tp->alpha_r <= 1.0) || !(tp->alpha_v > 0.0 && tp->alpha_v <= 1.0) ||
        !(tp->alpha_e > 0.0 && tp->alpha_e <= 1.0))
        return fail(ctx, RSP_ERR_ARG, "%s: alpha %g, %g, %g outside (0, 1]", who, tp->alpha_r, tp->alpha_v, tp->alpha_e);
    if (slots < 1 || slots > 65535) return fail(ctx, RSP_ERR_ARG, "%s: slots = %d outside 1..65535", who, slots);
    if (((uintptr_t)d_est | (uintptr_t)d_dt | (uintptr_t)d_state_f | (uintptr_t)d_snap_f) & 7)
        return fail(ctx, RSP_ERR_ARG, "%s: misaligned argument (doubles: 8 bytes)", who);
    if (((uintptr_t)d_count | (uintptr_t)d_slot | (uintptr_t)d_state_i | (uintptr_t)d_meta | (uintptr_t)d_assign |
         (uintptr_t)d_snap_i | (uintptr_t)d_tcount) & 3)
        return fail(ctx, RSP_ERR_ARG, "%s: misaligned argument (ints: 4 bytes)", who);
    const int64_t T = tp->max_tracks;
    // the table and one CPI's plots live in LDS (this also bounds the byte counts below)
    if (rsp::track_lds_bytes(T, max_hits) > rsp::track_lds_max())
        return fail(ctx, RSP_ERR_UNSUPPORTED,
                    "%s: max_tracks %d and max_hits %lld need %zu bytes of LDS (56 per entry, 32 per plot), over %zu", who,
                    tp->max_tracks, (long long)max_hits, rsp::track_lds_bytes(T, max_hits), rsp::track_lds_max());
    {
        struct Buf {
            const void* p;
            int64_t n;
        };
        const Buf bufs[] = {{d_est, batch * max_hits * 24},   {d_count, batch * 8},          {d_slot, batch * 4},
                            {d_dt, batch * 8},                {d_state_f, slots * T * 32},   {d_state_i, slots * T * 32},
                            {d_meta, (int64_t)slots * 8},     {d_assign, batch * max_hits * 4}, {d_snap_f, batch * T * 32},
                            {d_snap_i, batch * T * 32},       {d_tcount, batch * 32}};
        constexpr int nb = sizeof(bufs) / sizeof(bufs[0]);
        for (int i = 0; i < nb; ++i)
            for (int j = i + 1; j < nb; ++j)
                if (bufs[i].p && bufs[j].p && bufs[i].n > 0 && bufs[j].n > 0 &&
                    ranges_overlap(bufs[i].p, bufs[i].n, bufs[j].p, bufs[j].n))
                    return fail(ctx, RSP_ERR_ARG, "%s: buffers %d and %d overlap", who, i, j);
    }
    if (rsp::track_lds_bytes(T, max_hits) > rsp::track_lds_max())
        return fail(ctx, RSP_ERR_UNSUPPORTED,
                    "%s: max_tracks %d and max_hits %lld need %zu bytes of LDS (56 per entry, 32 per plot), over %zu", who,
                    tp->max_tracks, (long long)max_hits, rsp::track_lds_bytes(T, max_hits), rsp::track_lds_max());
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "%s: null ctx", who);
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    rsp::TrackArgs a{};
    a.T = tp->max_tracks;
    a.H = (int)max_hits;
    a.M = tp->confirm_m;
    a.N = tp->confirm_n;
    a.drop_t = tp->drop_tentative;
    a.drop_c = tp->drop_confirmed;
    a.slots = slots;
    a.dt = tp->dt;
    a.rate_sign = tp->rate_sign;
    a.gate_r = tp->gate_r;
    a.gate_v = tp->gate_v;
    a.wr = 1.0 / (tp->gate_r * tp->gate_r);
    a.wv = 1.0 / (tp->gate_v * tp->gate_v);
    a.alpha_r = tp->alpha_r;
    a.alpha_v = tp->alpha_v;
    a.alpha_e = tp->alpha_e;
    HIP_TRY(ctx, rsp::launch_track(d_est, d_count, batch, a, d_slot, d_dt, d_state_f, d_state_i, d_meta, d_assign,
                                   d_snap_f, d_snap_i, d_tcount, (hipStream_t)stream));
    return RSP_OK;
}

// ------------------------------------------------------------------ post-detection integration
// Both forms: everything is checked on the host before the context is looked at; `esz` is the element size
// (4: the sum form, 1: the binary form).
static int integ_check(rsp_ctx* ctx, const char* who, int esz, const void* d_in, int64_t V, int64_t R, int64_t batch,
                       const rsp_integ_params* ip, const int32_t* d_shift, const int32_t* d_slot, int32_t slots,
                       const void* d_hist, const int32_t* d_meta, const void* d_out, const int32_t* d_neff,
                       rsp::IntegArgs* a) {
    if (!ip || !d_in || !d_meta || !d_out)
        return fail(ctx, RSP_ERR_ARG, "%s: null %s", who, !ip ? "params" : !d_in ? "d_in" : !d_meta ? "d_meta" : "d_out");
    if (V < 1 || R < 1 || V > (1 << 20) || R > (1 << 20) || V * R > (int64_t)1 << 31 || batch < 0 || batch > 0x7fffffff)
        return fail(ctx, RSP_ERR_ARG, "%s: bad shape %lld x %lld x %lld", who, (long long)batch, (long long)V, (long long)R);
    if (ip->n < 1 || ip->n > RSP_INTEG_MAX_N)
        return fail(ctx, RSP_ERR_ARG, "%s: n = %d outside 1..%d", who, ip->n, RSP_INTEG_MAX_N);
    if (esz == 4 && (ip->m != 0 || ip->spread != 0))
        return fail(ctx, RSP_ERR_ARG, "%s: m = %d, spread = %d (both 0 in the sum form)", who, ip->m, ip->spread);
    if (esz == 1 && (ip->m < 1 || ip->m > ip->n))
        return fail(ctx, RSP_ERR_ARG, "%s: m = %d outside 1..n = %d", who, ip->m, ip->n);
    if (esz == 1 && (ip->spread < 0 || ip->spread > 2))
        return fail(ctx, RSP_ERR_ARG, "%s: spread = %d outside 0..2", who, ip->spread);
    if (ip->reserved != 0) return fail(ctx, RSP_ERR_ARG, "%s: reserved = %d", who, ip->reserved);
    const int64_t ld = ip->ld ? ip->ld : R, cs = ip->cpi_stride ? ip->cpi_stride : V * ld;
    if (ld < R || cs < (V - 1) * ld + R || (batch > 0 && cs > ((int64_t)1 << 60) / batch))
        return fail(ctx, RSP_ERR_ARG, "%s: row pitch %lld / CPI stride %lld too small for %lld x %lld", who, (long long)ld,
                    (long long)cs, (long long)V, (long long)R);
    if (slots < 1 || slots > 65535) return fail(ctx, RSP_ERR_ARG, "%s: slots = %d outside 1..65535", who, slots);
    if (ip->n > 1 && !d_hist) return fail(ctx, RSP_ERR_ARG, "%s: null d_hist with n = %d", who, ip->n);
    if (esz == 4 && (((uintptr_t)d_in | (uintptr_t)d_hist | (uintptr_t)d_out) & 3))
        return fail(ctx, RSP_ERR_ARG, "%s: misaligned plane (floats: 4 bytes)", who);
    if (((uintptr_t)d_shift | (uintptr_t)d_slot | (uintptr_t)d_meta | (uintptr_t)d_neff) & 3)
        return fail(ctx, RSP_ERR_ARG, "%s: misaligned argument (ints: 4 bytes)", who);
    // in place is not allowed: later CPIs of a batch read earlier input planes
    const int64_t span = batch > 0 ? ((batch - 1) * cs + (V - 1) * ld + R) * esz : 0;
    const int64_t hspan = d_hist ? (int64_t)slots * (ip->n - 1) * V * R * esz : 0;
    if (span > 0 && ranges_overlap(d_out, span, d_in, span)) return fail(ctx, RSP_ERR_ARG, "%s: d_out overlaps d_in", who);
    if (span > 0 && hspan > 0 && ranges_overlap(d_out, span, d_hist, hspan))
        return fail(ctx, RSP_ERR_ARG, "%s: d_out overlaps d_hist", who);
    if (span > 0 && hspan > 0 && ranges_overlap(d_in, span, d_hist, hspan))
        return fail(ctx, RSP_ERR_ARG, "%s: d_in overlaps d_hist", who);
    a->V = (int)V;
    a->R = (int)R;
    a->n = ip->n;
    a->m = ip->m;
    a->spread = ip->spread;
    a->slots = slots;
    a->ld = ld;
    a->cs = cs;
    return RSP_OK;
}

// The plan table from the context's pool (grow-only), ordered after the previous call's use of it.
static int integ_pool(rsp_ctx* ctx, int64_t batch, int n, hipStream_t st, int32_t** plan) {
    int rc = scratch_acquire(ctx, st);
    if (rc) return rc;
    if ((rc = ensure(ctx, ctx->integ_plan, rsp::integ_plan_bytes(batch, n))) != RSP_OK) return rc;
    *plan = (int32_t*)ctx->integ_plan.p;
    return RSP_OK;
}

int rsp_integrate_dev(rsp_ctx* ctx, const float* d_in, int64_t V, int64_t R, int64_t batch, const rsp_integ_params* ip,
                      const int32_t* d_shift, const int32_t* d_slot, int32_t slots, float* d_hist, int32_t* d_meta,
                      float* d_out, int32_t* d_neff, void* stream) {
    const char* who = "rsp_integrate_dev";
    rsp::IntegArgs a{};
    int rc = integ_check(ctx, who, 4, d_in, V, R, batch, ip, d_shift, d_slot, slots, d_hist, d_meta, d_out, d_neff, &a);
    if (rc) return rc;
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "%s: null ctx", who);
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    int32_t* plan = nullptr;
    if ((rc = integ_pool(ctx, batch, a.n, st, &plan))) return rc;
    HIP_TRY(ctx, rsp::launch_integ_sum(d_in, d_hist, d_shift, d_slot, d_meta, plan, d_out, d_neff, batch, a, st));
    return scratch_release(ctx, st);
}

int rsp_binint_dev(rsp_ctx* ctx, const uint8_t* d_in, int64_t V, int64_t R, int64_t batch, const rsp_integ_params* ip,
                   const int32_t* d_shift, const int32_t* d_slot, int32_t slots, uint8_t* d_hist, int32_t* d_meta,
                   uint8_t* d_out, int32_t* d_neff, void* stream) {
    const char* who = "rsp_binint_dev";
    rsp::IntegArgs a{};
    int rc = integ_check(ctx, who, 1, d_in, V, R, batch, ip, d_shift, d_slot, slots, d_hist, d_meta, d_out, d_neff, &a);
    if (rc) return rc;
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "%s: null ctx", who);
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    int32_t* plan = nullptr;
    if ((rc = integ_pool(ctx, batch, a.n, st, &plan))) return rc;
    HIP_TRY(ctx, rsp::launch_integ_bin(d_in, d_hist, d_shift, d_slot, d_meta, plan, d_out, d_neff, batch, a, st));
    return scratch_release(ctx, st);
}

// ------------------------------------------------------------------ stacked beams: fusion and elevation
// What both calls check about the shape, the parameters and the input planes, before the context is looked at.
static int fuse_check(rsp_ctx* ctx, const char* who, const float* d_amp, const uint8_t* d_flag, int64_t V, int64_t R,
                      int64_t batch, const rsp_fuse_params* fp, rsp::FuseArgs* a, int64_t* extent) {
    if (!fp || !d_amp || !d_flag)
        return fail(ctx, RSP_ERR_ARG, "%s: null %s", who, !fp ? "params" : !d_amp ? "d_amp" : "d_flag");
    if (V < 1 || R < 1 || V > (1 << 20) || R > (1 << 20) || V * R > (int64_t)1 << 31 || batch < 0 || batch > 0x7fffffff)
        return fail(ctx, RSP_ERR_ARG, "%s: bad shape %lld x %lld x %lld", who, (long long)batch, (long long)V, (long long)R);
    if (fp->beams < 2 || fp->beams > RSP_FUSE_MAX_BEAMS)
        return fail(ctx, RSP_ERR_ARG, "%s: beams = %d outside 2..%d", who, fp->beams, RSP_FUSE_MAX_BEAMS);
    if (fp->min_beams < 1 || fp->min_beams > fp->beams)
        return fail(ctx, RSP_ERR_ARG, "%s: min_beams = %d outside 1..beams = %d", who, fp->min_beams, fp->beams);
    if (fp->law < 0 || fp->law > 2) return fail(ctx, RSP_ERR_ARG, "%s: law = %d outside 0..2", who, fp->law);
    if (fp->reserved != 0) return fail(ctx, RSP_ERR_ARG, "%s: reserved = %d", who, fp->reserved);
    const int64_t beams = fp->beams;
    const int64_t ld = fp->ld ? fp->ld : R;
    if (ld < R || ld > ((int64_t)1 << 40))
        return fail(ctx, RSP_ERR_ARG, "%s: row pitch %lld for %lld columns", who, (long long)ld, (long long)R);
    const int64_t plane = (V - 1) * ld + R;   // the address range of one (CPI, beam) plane, in elements
    const int64_t bs = fp->beam_stride ? fp->beam_stride : V * ld;
    const int64_t cs = fp->cpi_stride ? fp->cpi_stride : beams * V * ld;
    const int64_t lim = (int64_t)1 << 56;
    bool ok = bs >= plane && bs <= lim / beams && (batch < 2 || (cs >= plane && cs <= lim / batch));
    if (ok && batch > 1) {
        const bool beam_inside = cs >= (beams - 1) * bs + plane;   // [batch][beams][V][ld]
        const bool cpi_inside = bs >= (batch - 1) * cs + plane;    // [beams][batch][V][ld]
        ok = beam_inside || cpi_inside;
    }
    if (!ok)
        return fail(ctx, RSP_ERR_ARG, "%s: beam stride %lld / CPI stride %lld: planes of %lld elements overlap (%lld beams, %lld CPIs)",
                    who, (long long)bs, (long long)cs, (long long)plane, (long long)beams, (long long)batch);
    for (int k = 0; k < fp->beams; ++k)
        if (!std::isfinite(fp->beam_el[k])) return fail(ctx, RSP_ERR_ARG, "%s: beam_el[%d] is not finite", who, k);
    const bool up = fp->beam_el[1] > fp->beam_el[0];
    for (int k = 1; k < fp->beams; ++k)
        if (up ? !(fp->beam_el[k] > fp->beam_el[k - 1]) : !(fp->beam_el[k] < fp->beam_el[k - 1]))
            return fail(ctx, RSP_ERR_ARG, "%s: beam_el is not strictly monotonic at %d", who, k);
    if ((uintptr_t)d_amp & 3) return fail(ctx, RSP_ERR_ARG, "%s: misaligned d_amp (floats: 4 bytes)", who);
    a->V = (int)V;
    a->R = (int)R;
    a->beams = fp->beams;
    a->min_beams = fp->min_beams;
    a->law = fp->law;
    a->ld = ld;
    a->bs = bs;
    a->cs = cs;
    for (int k = 0; k < RSP_FUSE_MAX_BEAMS; ++k) a->beam_el[k] = k < fp->beams ? fp->beam_el[k] : 0.0;
    *extent = batch > 0 ? (batch - 1) * cs + (beams - 1) * bs + plane : 0;   // elements from the base to the last cell
    return RSP_OK;
}

int rsp_beam_fuse_dev(rsp_ctx* ctx, const float* d_amp, const uint8_t* d_flag, int64_t V, int64_t R, int64_t batch,
                      const rsp_fuse_params* fp, uint8_t* d_fflag, uint8_t* d_fbeam, float* d_famp, uint8_t* d_fcnt,
                      void* stream) {
    const char* who = "rsp_beam_fuse_dev";
    rsp::FuseArgs a{};
    int64_t extent = 0;
    int rc = fuse_check(ctx, who, d_amp, d_flag, V, R, batch, fp, &a, &extent);
    if (rc) return rc;
    if (!d_fflag || !d_fbeam) return fail(ctx, RSP_ERR_ARG, "%s: null %s", who, !d_fflag ? "d_fflag" : "d_fbeam");
    if ((uintptr_t)d_famp & 3) return fail(ctx, RSP_ERR_ARG, "%s: misaligned d_famp (floats: 4 bytes)", who);
    const int64_t cells = batch * V * R;
    struct { const void* p; int64_t n; const char* name; } outs[] = {
        {d_fflag, cells, "d_fflag"}, {d_fbeam, cells, "d_fbeam"}, {d_famp, cells * 4, "d_famp"}, {d_fcnt, cells, "d_fcnt"}};
    for (int i = 0; i < 4 && cells > 0; ++i) {
        if (!outs[i].p) continue;
        if (ranges_overlap(outs[i].p, outs[i].n, d_amp, extent * 4) || ranges_overlap(outs[i].p, outs[i].n, d_flag, extent))
            return fail(ctx, RSP_ERR_ARG, "%s: %s overlaps an input", who, outs[i].name);
        for (int j = 0; j < i; ++j)
            if (outs[j].p && ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n))
                return fail(ctx, RSP_ERR_ARG, "%s: %s overlaps %s", who, outs[i].name, outs[j].name);
    }
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "%s: null ctx", who);
    if (batch == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(ctx, rsp::launch_beam_fuse(d_amp, d_flag, d_fflag, d_fbeam, d_famp, d_fcnt, batch, a, (hipStream_t)stream));
    return RSP_OK;
}

int rsp_beam_elev_dev(rsp_ctx* ctx, const float* d_amp, const uint8_t* d_flag, const uint8_t* d_fbeam, int64_t V, int64_t R,
                      int64_t batch, const rsp_fuse_params* fp, const int32_t* d_cells, const int32_t* d_count,
                      int64_t max_hits, double* d_el, int64_t el_stride, int32_t* d_hb, void* stream) {
    const char* who = "rsp_beam_elev_dev";
    rsp::FuseArgs a{};
    int64_t extent = 0;
    int rc = fuse_check(ctx, who, d_amp, d_flag, V, R, batch, fp, &a, &extent);
    if (rc) return rc;
    if (!d_fbeam || !d_count) return fail(ctx, RSP_ERR_ARG, "%s: null %s", who, !d_fbeam ? "d_fbeam" : "d_count");
    if (max_hits < 0 || max_hits > 0x7fffffff || el_stride < 1 || el_stride > (1 << 20))
        return fail(ctx, RSP_ERR_ARG, "%s: max_hits = %lld, el_stride = %lld", who, (long long)max_hits, (long long)el_stride);
    if (max_hits > 0 && (!d_cells || !d_el)) return fail(ctx, RSP_ERR_ARG, "%s: null %s", who, !d_cells ? "d_cells" : "d_el");
    if (rsp::beam_elev_blocks(batch, max_hits) > 0x7fffffff)
        return fail(ctx, RSP_ERR_ARG, "%s: %lld CPIs of %lld hits are more than 2^31 - 1 blocks of 256", who, (long long)batch,
                    (long long)max_hits);
    if (((uintptr_t)d_cells | (uintptr_t)d_count | (uintptr_t)d_hb) & 3)
        return fail(ctx, RSP_ERR_ARG, "%s: misaligned argument (ints: 4 bytes)", who);
    if ((uintptr_t)d_el & 7) return fail(ctx, RSP_ERR_ARG, "%s: misaligned d_el (doubles: 8 bytes)", who);
    if (!ctx) return fail(nullptr, RSP_ERR_ARG, "%s: null ctx", who);
    if (batch == 0 || max_hits == 0) return RSP_OK;
    if (!set_device(ctx)) return fail(ctx, RSP_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(ctx, rsp::launch_beam_elev(d_amp, d_flag, d_fbeam, d_cells, d_count, max_hits, d_el, el_stride, d_hb, batch, a,
                                       (hipStream_t)stream));
    return RSP_OK;
}
