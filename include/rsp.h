/*
 * rsp.h -- C ABI of the MI355X range-Doppler engine (pulse compression -> MTD ->
 * zero-velocity suppression -> 2-D CA-CFAR), the drop-in boundary for the hot path
 * of XuZerui2023/Radar-Signal-Process.
 *
 * Plain C linkage, plain pointers and int64 sizes; no C++ or torch types cross it.
 * Each entry point cites the MATLAB interface it replaces (paths relative to the
 * reference root):
 *
 *   rsp_pc_mtd        MTD_Signal = fun_MTD_produce(echoData, params)
 *                     (MTD/fun_MTD_produce.m:12; legacy 1-arg form
 *                      MatlabProcess_xuzerui/fun_MTD_produce.m:3; callers
 *                      MTD/main_produce_dataset_win_xzr_v2.m:136,
 *                      MatlabProcess_xuzerui/main_produce_dataset_win_xzr.m:37-38)
 *   rsp_cfar          [flag, flagV] = executeCFAR(rdm, refR, saveR, TR, mR,
 *                                                 refV, saveV, TV, mV, M0, rFlag)
 *                     (MatlabProcess_xuzerui/CFAR_WangCai/executeCFAR.m:1-2), and with
 *                     nseg > 1 the segmented cfarFlag = fun_CFARflag(...)
 *                     (CFAR_WangCai/main_cfar.m:142-161, a local function there),
 *                     optionally preceded by main_cfar.m:88-91's fun_0v_pressing
 *   rsp_pc_mtd_cfar   the fused chain fun_MTD_produce -> main_cfar's per-window CFAR
 *                     (MTD/main_produce_dataset_win_xzr_v2.m:136 then
 *                      CFAR_WangCai/main_cfar.m:88-93)
 *
 * Conventions
 *   - Every call returns an int status (RSP_OK = 0); the message of the last failure
 *     is rsp_last_error(ctx) (ctx == NULL: the last rsp_create failure).
 *   - Host-buffer entry points (no _dev suffix) are synchronous; the caller owns the
 *     host buffers, the context owns its device buffers (grow-only pool).
 *   - _dev entry points take device pointers and enqueue on `stream` (a hipStream_t,
 *     NULL = the null stream); they return before the work completes.
 *   - One context per host thread and device.  MATLAB calls MEX on one thread.  Contexts
 *     on different threads and devices are independent (kernel launch setup is cached per
 *     device, thread-safely).  _dev calls on one context may use different streams: each
 *     call's stream first waits for the previous call's use of the context's scratch.
 *   - Device layouts are row-major C order: echo [batch][P][R] complex (interleaved
 *     I/Q), RDM [batch][Nd][R_out] float32, flags [batch][Nd][R_out] uint8 0/1, where
 *     Nd = P (Doppler bins) and R_out = params.R_out.
 *   - Host-buffer entry points accept MATLAB column-major (RSP_COLMAJOR: element
 *     (p, r) at r*P + p) or row-major data and convert on the device.
 */
#ifndef RSP_H
#define RSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSP_ABI_VERSION 5   /* 2: rsp_set_fused / rsp_chain_check removed, rsp_set_pc_split added;
                               3: rsp_set_host_pipeline;
                               4: rsp_set_flow / rsp_flow_status (round 5's opt-in dataflow launch,
                                  with its RSP_K_FLOW profile slot) removed; rsp_set_range_concat
                                  added; rsp_profile_read_n
                                  takes the arrays' length, rsp_profile_read writes exactly the 4
                                  ABI-3 entries;
                               5: rsp_score_dev / rsp_score_summary with rsp_score_params and
                                  rsp_score_result added; rsp_integrate_dev / rsp_binint_dev with
                                  rsp_integ_params are an addition within 5, as are
                                  rsp_beam_fuse_dev / rsp_beam_elev_dev with rsp_fuse_params */
#define RSP_MAX_SEG 4
#define RSP_MAX_FIR_TAPS 64

typedef struct rsp_ctx rsp_ctx;

typedef enum {
    RSP_OK = 0,
    RSP_ERR_ARG = 1,          /* bad pointer / enum / size */
    RSP_ERR_SHAPE = 2,        /* P, R, batch inconsistent with the context's params */
    RSP_ERR_UNSUPPORTED = 3,  /* valid in MATLAB but not built here (e.g. odd FFT size) */
    RSP_ERR_CFAR_WINDOW = 4,  /* a CFAR window does not fit: MATLAB raises an index error */
    RSP_ERR_HIP = 5,          /* HIP runtime error (message has the HIP string) */
    RSP_ERR_NOMEM = 6
} rsp_status;

typedef enum {
    RSP_C64 = 0,        /* complex float32, interleaved re,im */
    RSP_C128 = 1,       /* complex float64, interleaved (MATLAB R2018a mxGetComplexDoubles) */
    RSP_C32F16 = 2      /* complex float16, interleaved (fp16 I/Q, fp32 compute) */
} rsp_dtype;

typedef enum {
    RSP_ROWMAJOR = 0,   /* [P][R]: one pulse (PRT) per row, range contiguous */
    RSP_COLMAJOR = 1    /* MATLAB P x R: [R][P], pulses contiguous */
} rsp_layout;

typedef enum {
    RSP_SEG_FIR = 0,    /* y = scale * filter(taps, 1, x) then circshift(y, -fir_shift)
                           (MTD/fun_lss_pulse_compression.m:38-51) */
    RSP_SEG_MF = 1      /* y[n] = sum_k x[n+k] * conj(s[k]), x zero past in_len and
                           periodic with period nfft (circular when in_len == nfft):
                           MTD/fun_pulse_compression.m:10-39 (linear, nfft >= in_len +
                           coef_len - 1) or DMX_SignalProcessing_main_xzr.m:348-352 */
} rsp_seg_kind;

typedef enum {
    RSP_WIN_KAISER = 0,   /* kaiser(P, window_beta)  (MTD/fun_Process_MTD.m:17-18) */
    RSP_WIN_HAMMING = 1,  /* hamming(P)  (DMX_SignalProcessing_main_xzr.m:211) */
    RSP_WIN_RECT = 2
} rsp_window;

typedef struct {
    int32_t kind;          /* rsp_seg_kind */
    int32_t fir_shift;     /* FIR: out[n] = z[(n + fir_shift) mod out_len] */
    int64_t in_start;      /* input columns [in_start, in_start + in_len) */
    int64_t in_len;
    int64_t out_start;     /* output columns [out_start, out_start + out_len) */
    int64_t out_len;       /* FIR: out_len == in_len; MF: out_len <= nfft */
    int64_t nfft;          /* MF: FFT length, a power of two, 64 <= nfft <= 16384 (anything
                              else: RSP_ERR_UNSUPPORTED) */
    double scale;          /* FIR: output scale (1/1.2 for the v2/legacy short pulse);
                              MF: replica scale */
    int64_t coef_len;      /* FIR: taps (<= RSP_MAX_FIR_TAPS); MF: replica length */
    const double* coef_re; /* FIR taps / MF replica real part (copied at rsp_create) */
    const double* coef_im; /* MF replica imaginary part (NULL = 0) */
} rsp_pc_segment;

typedef struct {
    int64_t P;             /* pulses per CPI, P >= 2.  The Doppler length V (mtd_nfft, or P) must be
                              a radix length -- 2^k, 16..2048, or 3*2^k, 48..1536 -- with any
                              P <= V; on one beam with mtd_nfft = 0 every other 2 <= P <= 1024 runs
                              by Bluestein.  Two beams: V = 512, 1024 or 2048.  Anything else:
                              RSP_ERR_UNSUPPORTED */
    int64_t R;             /* input range bins per pulse */
    int64_t R_out;         /* output range bins (PC output = RDM columns) */
    int32_t nseg;          /* pulse-compression segments (<= RSP_MAX_SEG) */
    int32_t window;        /* rsp_window for the slow-time FFT */
    double window_beta;    /* kaiser beta (8 in fun_Process_MTD) */
    int32_t fftshift;      /* 1: fftshift the Doppler axis (fun_Process_MTD.m:31) */
    int32_t zero_v_div;    /* fun_0v_pressing divisor (150 in MTD/fun_0v_pressing.m:22);
                              0 = no suppression */
    rsp_pc_segment seg[RSP_MAX_SEG];
    /* ---- DMX slow-time variant (DMX_SignalProcessing_main_xzr.m:208-229,414-426,462-465);
     *      all zero = the fun_Process_MTD path above ---- */
    int64_t mtd_nfft;      /* Doppler FFT length V (fft(pc.*w, V, 1)); 0 = P.  V > P zero-pads
                              the pulses (DMX mtd_FFT_num = 2048 over prtNum = 1536).  The RDM
                              and the CFAR work on V rows. */
    int32_t beams;         /* 0/1: one beam.  2: the DMX left/right pair -- echo [2][P][R] per
                              CPI (beam 0 = left), RDM = |X_L| + |X_R| (:421-422), optional
                              difference |X_R| - |X_L| (:425-426, rsp_pc_mtd_cfar_diff_dev) */
    int32_t zero_ends;     /* 0: off.  n > 0: zero RDM rows [0, n) and [V-n+1, V) -- the DMX
                              zeroSetFlagMTD with n = MTD_0_num + 1 (:463-465); replaces
                              fun_0v_pressing (zero_v_div) for the RDM */
} rsp_params;

typedef struct {
    int32_t refR, saveR, methodR;   /* range CFAR: reference, guard cells, 0 GO / 1 SO */
    double TR;                      /* range CFAR threshold factor */
    int32_t refV, saveV, methodV;   /* Doppler CFAR */
    double TV;
    int32_t M0;                     /* MTD_0_num: strips rows 1..M0+1 and V-M0+1..V */
    int32_t rFlag;                  /* 1: range CFAR on the Doppler hits; 0: flag = flagV */
    int32_t zero_v_div;             /* fun_0v_pressing before CFAR (20 in
                                       CFAR_WangCai/fun_0v_pressing.m:5); 0 = none */
    int32_t nseg;                   /* column segments; 0 = one segment, all columns */
    int64_t seg_lo[RSP_MAX_SEG];    /* 0-based [seg_lo, seg_hi); columns outside every
                                       segment get flag 0 (main_cfar.m:156-159) */
    int64_t seg_hi[RSP_MAX_SEG];
} rsp_cfar_params;

/* Library version string, e.g. "rsp-mi355x 0.1.0 (gfx950)". */
const char* rsp_version(void);

/* Create a context bound to HIP device `device` for one parameter set.  Builds the
 * matched-filter spectra (fp64 on the host, stored fp32), twiddle tables and window.
 * params == NULL creates a CFAR-only context (rsp_cfar / rsp_cfar_dev). */
int rsp_create(rsp_ctx** out, int device, const rsp_params* params);

/* Context for fun_MTD_produce v2 built from its `params` fields (MTD/fun_MTD_produce.m:
 * 34-69, MTD/main_produce_dataset_win_xzr_v2.m:31-45): P = prtNum, R = echo width,
 * point_prt = {total, p1, p2, p3}, fs [Hz], B [Hz], tao = {tau1, tau2, tau3} [s].
 * Synthesises pulse2 = exp(j*pi*(-B/tau2)*t^2) and pulse3 = exp(j*pi*(B/tau3)*t^2) with
 * t = -tau/2 : 1/fs : tau/2-1/fs, the 35-tap FIR /max /1.2 with its 17-sample group-delay
 * circshift, kaiser(P, 8) + fftshift MTD and fun_0v_pressing /150. */
int rsp_create_v2(rsp_ctx** out, int device, int64_t P, int64_t R, const int64_t point_prt[4],
                  double fs, double B, const double tao[3]);
/* Context for the legacy one-argument MTD_Signal = fun_MTD_produce(echo)
 * (MatlabProcess_xuzerui/fun_MTD_produce.m:3-126; called at main_produce_dataset_win_xzr.m:37-38):
 * P = prtNum, R = echo width, the hard-coded split 82 / 242 / R-324 (:24-38), the 35-tap FIR
 * /max /1.2 with no group-delay shift, the two measured pulses the .m file holds inline
 * (pulse2: n2 samples, pulse3: n3 samples, as separate real / imaginary arrays -- the shim
 * reads them from the repository's data files), kaiser(P, 8) + fftshift MTD, 0-v /150. */
int rsp_create_legacy(rsp_ctx** out, int device, int64_t P, int64_t R, const double* pulse2_re,
                      const double* pulse2_im, int64_t n2, const double* pulse3_re, const double* pulse3_im,
                      int64_t n3);
int rsp_destroy(rsp_ctx* ctx);
const char* rsp_last_error(const rsp_ctx* ctx);

/* CPIs processed per internal chunk (PC scratch = chunk * P * R_out * 8 bytes, sized to
 * stay in the 256 MiB Infinity Cache).  0 restores the default.  Window mode counts output
 * windows: chunk / windows frame pairs per chunk (each chunk also pulse-compresses one
 * look-ahead frame); the default there is at least 32 pairs (fewer look-ahead frames and
 * launches beat Infinity-Cache residency for the window stream). */
int rsp_set_chunk(rsp_ctx* ctx, int64_t cpis_per_chunk);

/* Per-pipeline chunk sizes (an addition within ABI 5).  Chunk k of a chain call runs on pipeline
 * k % n; with this call pipeline i's chunks are cpis[i] CPIs each, so the batch is cut cpis[0],
 * cpis[1], ..., cpis[n-1], cpis[0], ... and only the final chunk is short.  Pipelines of unequal
 * chunks have unequal periods, so their PC / MTD phases cannot lock.  1 <= n <= 4 sets both the
 * sizes and the pipeline count of non-window chains (as rsp_set_streams(n) would); n = 0 restores
 * the default.  A later rsp_set_chunk with a size > 0 means equal chunks again.  Window mode is
 * unaffected.  Results do not depend on the chunking.  Per-pipeline scratch is sized by the
 * largest chunk: n * max(cpis) * P * R_out * 8 bytes of PC scratch, and with a range
 * concatenation as much again times pc_width / R_out for its staging rows. */
int rsp_set_lane_chunks(rsp_ctx* ctx, const int64_t* cpis, int32_t n);

/* Number of chunk pipelines (1..4; 0 = the default: 2, window mode 1): chunk k runs on the
 * caller's stream or on one of n-1 context-owned streams that fork from and join back into
 * it, so consecutive chunks overlap.  Each pipeline owns one PC scratch slot (n = 1: every
 * launch alone, for per-kernel timing). */
int rsp_set_streams(rsp_ctx* ctx, int32_t n);

/* Device memory a chain context holds (grow-only pools, freed by rsp_destroy), per call shape:
 *   PC scratch        pipelines x chunk x beams x P x R_out x 8 B (c3: 2 x 16 x 128 x 4096 x 8 = 128 MiB)
 *   hit-list slots    the grouped range stage keeps up to 16 chunks' Doppler-hit lists per
 *                     pipeline, each MTD workgroup's region sized to its own cells (no overflow
 *                     possible): pipelines x 16 x chunk x V x R_out x 4 B, capped at 1 GiB
 *                     (c3: exactly 1 GiB; c5, one-CPI chunks: 2 x 16 x 32 MiB = 1 GiB)
 *   host-call staging the host-buffer entry points' device copies of their inputs / outputs
 * i.e. ~1.2 GiB per context at c3, against 288 GB of HBM; rsp_set_chunk scales all three. */

/* ---- host-buffer entry points (MEX / fun_MTD_produce drop-in), synchronous ---------- */
/* rsp_pc_mtd_cfar / rsp_pc_mtd take pageable host buffers (MATLAB's arrays).  A call that fits
 * one chunk (every MATLAB-granularity call) is staged through pinned memory that the kernels
 * read and write directly across PCIe: the host copy threads convert ~1 MiB input pieces while
 * the transpose kernels consume the earlier ones, and deliver ~1 MiB output parts while the later
 * parts cross the link.  A larger batch is pipelined in chunks of CPIs: chunk k's host->device
 * copy, chain and device->host copy overlap chunks k+1 and k-1 (two copy streams beside the
 * context's stream), staged through rings of 8 MiB pinned pieces copied by the thread pool.
 * Outputs are identical to the _dev path's. */
/* CPIs per host chunk (0 = by size: 32 MiB of device-side input, 8 CPIs at 128 x 4096) and
 * host copy threads (0 = default: 8 with >= 16 hardware threads). */
int rsp_set_host_pipeline(rsp_ctx* ctx, int64_t cpis_per_chunk, int32_t copy_threads);

int rsp_pc_mtd(rsp_ctx* ctx, const void* echo, int32_t dtype, int32_t layout,
               int64_t P, int64_t R, int64_t batch, float* rdm_out, int32_t rdm_layout);

int rsp_cfar(rsp_ctx* ctx, const float* rdm, int32_t rdm_layout, int64_t V, int64_t R,
             int64_t batch, const rsp_cfar_params* cfar, uint8_t* flag_out,
             uint8_t* flagV_out /* nullable */);

int rsp_pc_mtd_cfar(rsp_ctx* ctx, const void* echo, int32_t dtype, int32_t layout,
                    int64_t P, int64_t R, int64_t batch, const rsp_cfar_params* cfar,
                    float* rdm_out /* nullable */, int32_t out_layout, uint8_t* flag_out,
                    uint8_t* flagV_out /* nullable */);

/* MATLAB-typed forms for the MEX drop-ins (replacing the .m functions' own double outputs,
 * MTD/fun_MTD_produce.m:12 and CFAR_WangCai/executeCFAR.m:1-2): as rsp_pc_mtd_cfar / rsp_cfar,
 * but the RDM and the 0/1 flags land as double and the CFAR input is double.  The widening
 * (float -> double, byte -> double) and narrowing (double -> float, round to nearest) run on
 * the host copy threads, piece by piece as each pinned piece or part lands, instead of in a
 * serial loop in the shim.  Values are identical to the float / byte forms'.  rsp_pc_mtd_cfar_f64
 * with cfar == NULL is fun_MTD_produce. */
int rsp_pc_mtd_cfar_f64(rsp_ctx* ctx, const void* echo, int32_t dtype, int32_t layout,
                        int64_t P, int64_t R, int64_t batch, const rsp_cfar_params* cfar,
                        double* rdm_out /* nullable */, int32_t out_layout, double* flag_out,
                        double* flagV_out /* nullable */);
int rsp_cfar_f64(rsp_ctx* ctx, const double* rdm, int32_t rdm_layout, int64_t V, int64_t R,
                 int64_t batch, const rsp_cfar_params* cfar, double* flag_out,
                 double* flagV_out /* nullable */);

/* ---- device-pointer entry points, asynchronous on `stream` -------------------------- */
/* d_echo: [batch][P][R] rsp_dtype RSP_C64 or RSP_C32F16.  cfar == NULL: PC + MTD only.
 * d_rdm may be NULL only when cfar != NULL (then an internal buffer is used). */
int rsp_pc_mtd_cfar_dev(rsp_ctx* ctx, const void* d_echo, int32_t dtype, int64_t batch,
                        const rsp_cfar_params* cfar, float* d_rdm, uint8_t* d_flag,
                        uint8_t* d_flagV, void* stream);

int rsp_cfar_dev(rsp_ctx* ctx, const float* d_rdm, int64_t V, int64_t R, int64_t batch,
                 const rsp_cfar_params* cfar, uint8_t* d_flag, uint8_t* d_flagV,
                 void* stream);

/* The chain after pulse compression (fun_Process_MTD + fun_0v_pressing + executeCFAR) on
 * already pulse-compressed rows, e.g. from rsp_pc_dev: d_pc [batch][beams][P][R_out] RSP_C64.
 * Outputs as rsp_pc_mtd_cfar_dev. */
int rsp_mtd_cfar_dev(rsp_ctx* ctx, const void* d_pc, int64_t batch, const rsp_cfar_params* cfar,
                     float* d_rdm, uint8_t* d_flag, uint8_t* d_flagV, void* stream);

/* rsp_pc_mtd_cfar_dev for a two-beam context (rsp_params.beams == 2): d_echo
 * [batch][2][P][R]; d_sum [batch][V][R_out] = |X_L| + |X_R| (the RDM, zeroSetFlagMTD
 * applied); d_diff (nullable) = |X_R| - |X_L|; CFAR runs on the sum
 * (DMX_SignalProcessing_main_xzr.m:414-472). */
int rsp_pc_mtd_cfar_diff_dev(rsp_ctx* ctx, const void* d_echo, int32_t dtype, int64_t batch,
                             const rsp_cfar_params* cfar, float* d_sum, float* d_diff,
                             uint8_t* d_flag, uint8_t* d_flagV, void* stream);

/* Sliding-window stream (MTD/main_produce_dataset_win_xzr_v2.m:94-144; replaces its
 * beam x window loop of fun_MTD_produce calls at :117-136).  d_frames: [beams][frames+1][P][R]
 * consecutive frames of each beam.  For frame pair (n, n+1) and window i < win, the CPI is rows
 * [s_i, s_i + P) of [frame n; frame n+1] with s_i = round(i*P/win) (0-based, :123).  Outputs
 * [beams][frames][win][P][R_out] (MTD_win_all_beams{b}(i+1,:,:) per frame, :131-139); with
 * cfar != NULL each window also runs executeCFAR (flags in the same layout).  Pulse
 * compression is row-wise, so each frame's PC is computed once and shared by its windows
 * (exact).  win <= 16. */
int rsp_window_pc_mtd_cfar_dev(rsp_ctx* ctx, const void* d_frames, int32_t dtype, int64_t beams,
                               int64_t frames, int32_t win, const rsp_cfar_params* cfar,
                               float* d_rdm, uint8_t* d_flag, uint8_t* d_flagV, void* stream);

/* Pulse compression alone (fun_lss_pulse_compression), for tests and staged use:
 * d_pc = [batch][P][R_out] complex float32. */
int rsp_pc_dev(rsp_ctx* ctx, const void* d_echo, int32_t dtype, int64_t batch, void* d_pc,
               void* stream);

/* ---- execution strategy ------------------------------------------------------------------ */
/* Overlap-save split of long matched filters (default on): a segment whose FFT exceeds 4096
 * points, with no output that wraps, runs as 2048..8192-point overlap-save blocks instead of
 * one whole-length transform (the same correlation sums; results differ by fp32 rounding).
 * enable = 0 selects the whole-length transforms.  The threshold is fixed (4096 points).
 * RSP_ERR_UNSUPPORTED on a context without the specialised PC kernels (nothing to select). */
int rsp_set_pc_split(rsp_ctx* ctx, int32_t enable);

/* Pruned pulse-compression kernels (default on; an addition within ABI 5): where a matched
 * filter's rows end in whole 1/16-transform slices that are zero padding (input) or are cut by
 * out_len (output), a kernel instance built for the built-in presets skips those slices' loads,
 * stores and butterfly operations.  Every stored value is unchanged, except that an exact zero
 * may come out with the other sign.  enable = 0 runs the generic instances (for A/B runs and
 * tests).  Shapes without a built instance run the generic one either way.
 * RSP_ERR_UNSUPPORTED on a context without the specialised PC kernels (nothing to select). */
int rsp_set_pc_prune(rsp_ctx* ctx, int32_t enable);

/* Rows per workgroup of the 4096-point pulse-compression rows (additions within ABI 5): with
 * n = 2 or 4 a workgroup of those rows (v2 at 4096 range bins and above, DMX at 4096) runs n
 * consecutive rows -- or overlap-save blocks -- one after the other and loads the replica spectrum
 * and the twiddles once for all of them, not once per row.  n = 1 is one row per workgroup;
 * n = 0 returns to the library default.  Every stored value is bit-identical for every n.
 * Other row lengths, and 4096-point rows whose launch also runs the FIR segment, keep one row per
 * workgroup whatever n is.
 * RSP_ERR_UNSUPPORTED on a context without the specialised PC kernels; RSP_ERR_ARG for any other n. */
int rsp_set_pc_rows(rsp_ctx* ctx, int32_t n);
/* The rows per workgroup the context's next pulse-compression launch of 4096-point rows will run
 * (1, 2 or 4: the launcher's own choice); 1 where no launch takes the multi-row path. */
int rsp_get_pc_rows(rsp_ctx* ctx);

/* The pulse-compression launches the context will issue, as chosen from the segment lengths and
 * the two switches above (read-only; an addition within ABI 5) -- for tests and tools that must
 * know which kernel path a geometry takes.  One entry per matched-filter segment, in segment
 * order; the FIR segment rides on the first one's rows (fir = 1). */
typedef struct {
    int32_t nfft;      /* transform length the kernel runs: the segment's nfft, or the overlap-save
                          block length when nsub >= 1 */
    int32_t nsub;      /* overlap-save blocks per row; 0: the whole segment in one transform */
    int32_t sub_step;  /* outputs per overlap-save block (nfft - replica length + 1); 0 with nsub 0 */
    int32_t zin;       /* trailing 1/16-transform slices that are zero padding in every block ... */
    int32_t zout;      /* ... and that lie past the stored outputs in every block; both 0 for rows
                          shorter than 1024 points and with rsp_set_pc_prune(ctx, 0) */
    int32_t fir;       /* 1: this segment's launch also runs the FIR segment */
} rsp_pc_plan_seg;
typedef struct {
    int32_t specialised;   /* 1: the per-segment kernels; 0: the generic kernel, one workgroup per
                              row for all segments (every other field is then 0) */
    int32_t fused;         /* 1: both matched filters in one launch (a built pair of lengths) */
    int32_t prune;         /* pruned instance selected, hex digits <zin1><zout1><zin2><zout2> of the
                              slices it skips (0x4433, 0x4402); 0: the generic instance */
    int32_t nmf;           /* matched-filter segments = entries of seg[] filled */
    rsp_pc_plan_seg seg[RSP_MAX_SEG];
} rsp_pc_plan_t;
/* n: the seg[] entries `out` has room for (RSP_MAX_SEG for the struct above); RSP_ERR_ARG when
 * the context has more matched-filter segments than that. */
int rsp_pc_plan(rsp_ctx* ctx, rsp_pc_plan_t* out, int32_t n);

/* The CFAR kernels a call would run (read-only; an addition within ABI 5), from the same host
 * predicates the launchers use -- for tests and tools that must know which path a shape, a window
 * and a chunk plan take.  Nothing is launched and no buffer is touched. */
enum { RSP_CFAR_R_COPY = 0,      /* rFlag == 0: flag = flagV */
       RSP_CFAR_R_GENERIC = 1,   /* any window: one workgroup per row, the row staged in LDS */
       RSP_CFAR_R_4CELL = 2,     /* ref 5 / guard 7, R % 4 == 0: four cells per thread */
       RSP_CFAR_R_16CELL = 3 };  /* ref 5 / guard 7, R % 16 == 0: sixteen cells per thread */
enum { RSP_RANGE_NONE = 0,       /* rFlag == 0: the MTD launch writes flag = flagV */
       RSP_RANGE_GROUPED = 1,    /* one hit-list launch behind up to 16 chunks of a pipeline */
       RSP_RANGE_JOB57 = 2,      /* inside the pipeline's next MTD launch: a region's first `threads`
                                    hits with the tile's loads, the rest in a tail after the tile */
       RSP_RANGE_PREV_HITS = 3,  /* inside the pipeline's next MTD launch, after its tile */
       RSP_RANGE_PER_CHUNK = 4 };/* a hit-list launch behind every chunk's MTD */
enum { RSP_HITS_NONE = 0,
       RSP_HITS_BATCHED57 = 1,       /* ref 5 / guard 7, hit_lanes lanes per region */
       RSP_HITS_PER_HIT57 = 2,       /* ref 5 / guard 7, a workgroup per region, a thread per hit */
       RSP_HITS_PER_HIT_RUNTIME = 3 };/* any window, likewise */
typedef struct {
    int32_t fused;            /* the call asked about: 0 rsp_cfar / rsp_cfar_dev, 1 the chain */
    /* fused == 0 (the chain's fields are 0) */
    int32_t v_tile_log2;      /* log2 of the Doppler kernel's tile width in range bins */
    int32_t r_kernel;         /* RSP_CFAR_R_* */
    int32_t r_groups;         /* workgroups per row of the 4- / 16-cell kernels, else 0 */
    /* fused == 1 (the three fields above are 0) */
    int32_t window_compiled;  /* 1: the Doppler window is compiled into the MTD kernel (5 + 7) */
    int32_t bluestein;        /* Bluestein convolution length, 0 for a radix transform */
    int32_t tile_w;           /* range bins per MTD workgroup */
    int32_t threads;          /* threads per MTD workgroup */
    int32_t region;           /* hit-list entries per workgroup = tile_w * P */
    int32_t nchunks;          /* MTD launches of the call */
    int32_t nlanes;           /* chunk pipelines used */
    int32_t lane_chunk[4];    /* CPIs of a full chunk of each pipeline (0: pipeline unused) */
    int32_t lane_last[4];     /* CPIs of each pipeline's last chunk (the call's final chunk may be short) */
    int32_t range_stage;      /* RSP_RANGE_*: where a chunk's range stage runs; a pipeline's last chunk
                                 (and with RSP_RANGE_GROUPED every group) gets a hit-list launch */
    int32_t hit_kernel;       /* RSP_HITS_* of those launches (sized for the largest one) */
    int32_t hit_lanes;        /* lanes per region of RSP_HITS_BATCHED57 (16, 32, 64, 256), else 0 */
    int32_t flag_memset;      /* 1: the flag background is a memset, 0: the MTD kernel's stores */
} rsp_cfar_plan_t;
/* V, R, batch and cfar as for the call itself.  fused = 0: rsp_cfar_dev(ctx, ..., V, R, batch, cfar).
 * fused = 1: rsp_mtd_cfar_dev / rsp_pc_mtd_cfar_dev(ctx, ..., batch, cfar) with (with_rdm != 0) or
 * without a caller's RDM buffer; V and R must be the context's Doppler rows and R_out.  Returns
 * what that call's validation would return (RSP_ERR_ARG, RSP_ERR_CFAR_WINDOW, RSP_ERR_UNSUPPORTED). */
int rsp_cfar_plan(rsp_ctx* ctx, int64_t V, int64_t R, int64_t batch, const rsp_cfar_params* cfar,
                  int32_t fused, int32_t with_rdm, rsp_cfar_plan_t* out);

/* Range concatenation between pulse compression and the MTD, replacing
 *   Echo_0 = fun_lss_range_concate(prtNum, Echo_0)
 * (MatlabProcess_xuzerui/fun_lss_range_concate.m:4-7, called at main.m:210-211 -- and commented
 * out in the legacy fun_MTD_produce.m:70): after pulse compression, each row becomes the
 * concatenation of its columns [src_start[i], src_start[i] + len[i]), i < nparts, in order; the
 * MTD, the CFAR and every output then have R_out = sum(len) columns (rsp_pc_dev returns the
 * concatenated rows, rsp_mtd_cfar_dev takes them).  The reference's ranges are
 * {0, 89, 481} / {82, 236, 550} (1-based 1:82, 90:325, 482:1031 of the 1031 PC columns ->
 * 868, the width fun_CFARflag's hard-coded 1:82 | 83:318 | 319:868 split assumes,
 * main_cfar.m:143-145).  nparts = 0 restores the PC width.  Parts must lie inside the
 * params' R_out columns; nparts <= RSP_MAX_SEG. */
int rsp_set_range_concat(rsp_ctx* ctx, int32_t nparts, const int64_t* src_start, const int64_t* len);

/* ---- raw-data ingest --------------------------------------------------- */
/* One frame of the radar's PRT record stream -> DBF beams, replacing the per-PRT loop of
 *   [sig_data_DBF_allprts, servo_angle, frameCompleted, is_global_stream_end] =
 *       FrameDataRead_xzr(orgDataFilePath, DBF_coeffs_data_C, Sig_Config, frameRInd)
 * (FrameDataRead_xzr.m:20-204, called at bin_to_mat_xzr.m:62).  The host reads the frame's
 * bytes from the cross-file stream (read_continuous_file_stream.m; rsp/ingest.py mirrors it)
 * and this call parses and beamforms them on the GPU.  Record = head (bytes_head, uint32
 * fields), realtime block, payload padded to 64 B (DDC: int16 I/Q [sample][channel][I,Q]),
 * tail; in rsp_ingest_ddc_dev every PRT has the DDC record size (rsp_ingest_record_bytes).
 * Output (DDC): d_out[b * beam_stride + prt * point_prt + s] = sum_c (I + jQ)[s][c] * dbf[b][c]
 * (sig_data_C * DBF_coeffs_data_C.', :158) as complex64, beam-major so each beam is the
 * [prt][sample] echo the chain reads; beam_stride = 0 means prt_num * point_prt (pass a larger
 * stride to land frames in a [beam][frames+1][P][R] window buffer).
 * d_status: int32[prt_num + 1], per-PRT RSP_PRT_* codes, and [prt_num] = rows decoded: the
 * frame stops at the first PRT the reference would return at (those rows and all later ones
 * are written as zeros, servo 0), so frameCompleted == (status[prt_num] == prt_num && no
 * RSP_PRT_TAIL_TRUNCATED).  rsp_ingest_ddc_dev decodes DDC payloads (data_type 1) only, every
 * record sized by the params; rsp_ingest_frame_dev decodes every data type the reference
 * parses, each record sized by its own head (:104-119), so a frame may mix types:
 *   ADC (0): the int16 (samples x channels) matrix itself (:144-147) -- passes the size check
 *            only with channel_num (of the head) == beam_num; beam b = (x_b, 0);
 *   DBF (any other type): the 24-bit branch (:130-135,162-164) as MATLAB evaluates it -- its
 *            data_temp is uint8, so b0 + b1*2^8 + b2*2^16 saturates to 255 once b1 or b2 is
 *            non-zero (else b0) and the sign fix never fires; beam b = (v_2b, v_2b+1).  The
 *            sizes pass only when the value count (2*ch for ch % 4 == 1, 2*ch + 2 for
 *            ch % 4 == 0) is 2*beam_num; other channel counts are a MATLAB size error there and
 *            RSP_PRT_BAD_SHAPE here.  (The reference marks this branch unfinished.)
 * The two calls share per-context scratch: one frame at a time per context. */
typedef struct {
    int32_t prt_num;         /* Sig_Config.prtNum (332) */
    int32_t point_prt;       /* Sig_Config.point_PRT (3404) */
    int32_t channel_num;     /* Sig_Config.channel_num (16) */
    int32_t beam_num;        /* Sig_Config.beam_num (13) */
    int32_t bytes_head;      /* Sig_Config.bytesFrameHead (64) */
    int32_t bytes_realtime;  /* Sig_Config.bytesFrameRealtime (128) */
    int32_t bytes_tail;      /* Sig_Config.bytesFrameEnd (64) */
} rsp_ingest_params;

enum {
    RSP_PRT_OK = 0,
    RSP_PRT_TRUNCATED = 1,        /* head, realtime block or payload cut by the end of the stream */
    RSP_PRT_TAIL_TRUNCATED = 2,   /* decoded, but the tail is cut: the frame ends incomplete */
    RSP_PRT_BAD_COUNT = 3,        /* pulse_data_num <= 0 (FrameDataRead_xzr.m:90-94) */
    RSP_PRT_BAD_SHAPE = 4,        /* pulse_data_num != point_prt or channels != channel_num */
    RSP_PRT_UNSUPPORTED_TYPE = 5  /* data_type != 1 (DDC) in rsp_ingest_ddc_dev */
};

/* Bytes of one DDC PRT record of this shape. */
int rsp_ingest_record_bytes(const rsp_ingest_params* p, int64_t* bytes);
/* d_stream: nbytes of the frame's records (fewer than prt_num records: the rest are
 * truncated); d_dbf: float32 [beam_num][channel_num][2] (re, im); d_servo nullable. */
int rsp_ingest_ddc_dev(rsp_ctx* ctx, const uint8_t* d_stream, int64_t nbytes, const rsp_ingest_params* p,
                       const float* d_dbf, void* d_out, int64_t beam_stride, uint16_t* d_servo,
                       int32_t* d_status, void* stream);
/* Every data type, records sized by their heads (the same arguments; d_dbf is read by DDC
 * records only). */
int rsp_ingest_frame_dev(rsp_ctx* ctx, const uint8_t* d_stream, int64_t nbytes, const rsp_ingest_params* p,
                         const float* d_dbf, void* d_out, int64_t beam_stride, uint16_t* d_servo,
                         int32_t* d_status, void* stream);

/* ---- legacy two-beam 24-bit records (frameDataRead_A) ------------------------------------ */
/* nframes x prt_num consecutive PRT records of the legacy capture format -> the left and right
 * beams' echo planes, replacing the per-PRT loop of
 *   [echoData_Frame_Left, echoData_Frame_Right, frameInd, modFlag, beamPosNum, beamNums, freInd,
 *    angleCodeSeries] = frameDataRead_A(orgDataFilePath, frameRInd, prtNum)
 * (MatlabProcess_xuzerui/frameDataRead_A_xzr.m:53-148; Show_Read.m:49-142 is the two-argument
 * form that DMX_SignalProcessing_main_xzr.m:307 calls).  A record is 28 + 12 * point_prt + 8
 * bytes: two uint16 sync words (0xA5A5, never checked by the reference), frameInd as two uint16
 * (high word first), modFlag (uint16), beamPosNum, beamNums (uint8), freInd, prtInd (uint16), 10
 * skipped bytes, two angle bytes with angleCode = (b26 + b27 * 2^7) * 360 / 16384 (2^7 as the
 * reference writes it), then point_prt groups of 12 bytes [Ql Il Qr Ir] high, middle and low
 * bytes, then an 8-byte tail.  A sample is hi * 2^16 + mid * 2^8 + lo, minus 2^24 if it is
 * > 2^23 (:112-129): 0x800000 decodes to +8388608.  Left = I_l + j Q_l, Right = I_r + j Q_r.
 * Output: d_out[f * frame_stride + b * beam_stride + prt * point_prt + s] as complex64, b = 0
 * Left, 1 Right (strides in complex elements).  beam_stride = 0 means prt_num * point_prt and
 * frame_stride = 0 means 2 * beam_stride: the dense [nframes][2][prt_num][point_prt] tensor
 * that rsp_pc_mtd_cfar_diff_dev takes.  frame_stride = prt_num * point_prt with beam_stride =
 * nframes * prt_num * point_prt gives two [nframes][prt_num][point_prt] stacks.  The 2 * nframes
 * planes must not overlap: either beam_stride >= plane and frame_stride >= beam_stride + plane,
 * or frame_stride >= plane and beam_stride >= (nframes - 1) * frame_stride + plane; other
 * strides are refused.
 * d_angle: float64 [nframes][prt_num] angleCode per PRT, nullable.
 * d_head: int32 [nframes][prt_num][RSP_LEGACY_HEAD_FIELDS] = frameInd (its 32 bits), modFlag,
 * beamPosNum, beamNums, freInd, prtInd, sync_ok (both sync words are 0xA5A5), 0; nullable.  The
 * scalars frameDataRead_A returns are those of a frame's last PRT.
 * d_status: int32 [nframes * prt_num + 1], a RSP_PRT_* code per row (rows are frame x PRT in
 * stream order) and, last, the number of rows decoded.  RSP_PRT_TRUNCATED: the head or the
 * payload is cut by nbytes; that row and every later one are written as zeros, with angle 0 and
 * a zero head.  RSP_PRT_TAIL_TRUNCATED: only the 8 tail bytes are cut; the row is decoded (the
 * reference stores the row before it skips the tail).
 * Contract: d_stream is 4-byte aligned (the payload is read as dwords; a record is a multiple
 * of 4 bytes), d_out and d_angle 8-byte aligned; prt_num, nframes <= 65535, point_prt <= 2^24.
 * Arguments are checked before the context is touched (RSP_ERR_ARG with a message).  No context
 * scratch is used: calls on different streams do not interfere. */
typedef struct {
    int32_t prt_num;     /* prtNum (1536) */
    int32_t point_prt;   /* point_PRT (1031; 566 for the DMX waveform) */
    int32_t nframes;     /* consecutive frames in d_stream, >= 1 */
    int32_t reserved;    /* 0 */
} rsp_legacy_ingest_params;

enum { RSP_LEGACY_HEAD_FIELDS = 8 };  /* frameInd, modFlag, beamPosNum, beamNums, freInd, prtInd, sync_ok, 0 */

/* Bytes of one record: 28 + 12 * point_prt + 8. */
int rsp_legacy_record_bytes(const rsp_legacy_ingest_params* p, int64_t* bytes);
int rsp_ingest_legacy_dev(rsp_ctx* ctx, const uint8_t* d_stream, int64_t nbytes,
                          const rsp_legacy_ingest_params* p, void* d_out,
                          int64_t beam_stride, int64_t frame_stride,
                          double* d_angle, int32_t* d_head, int32_t* d_status, void* stream);

/* ---- post-detection measurement --------------------------------------- */
/* Range / velocity / elevation of every CFAR hit, replacing
 *   [rEstSeries, vEstSeries, eleAngleEstSeries] = motionParaMeasure(echo_MTD_sum, echo_MTD_diff,
 *       cfarResultFlag, extraDots, rScale, deltaR, rInterpTimes, vScale, deltaV, vInterpTimes,
 *       kValues, beamPosNum, beamAngleStep, freInd, eleAngleComp, eleAngleSysErr, MTD_0_num)
 * (MatlabProcess_xuzerui/CFAR_WangCai/motionParaMeasure.m:1-88, called at
 * DMX_SignalProcessing_main_xzr.m:489-494) for a batch of CPIs.  d_sum / d_diff: float32
 * [batch][V][R] (rsp_pc_mtd_cfar_diff_dev's d_sum / d_diff), d_flag: uint8 [batch][V][R]
 * (its d_flag); d_r_scale: float64 [R] (rScale), d_v_scale: float64 [V] (vScale).
 * Hit i of a CPI, in MATLAB's find() order (column-major: range bin, then Doppler row), gets
 * d_est[(cpi*max_hits + i)*3 + {0,1,2}] = {rEst, vEst, eleAngleEst} (float64) and, when
 * d_cells != NULL, d_cells[(cpi*max_hits + i)*2 + {0,1}] = its 0-based (row, column).
 * d_count[cpi*2] = hits in the CPI (only the first max_hits are written), d_count[cpi*2+1] =
 * hits the reference stops at with an index error (a hit too close to an edge for the
 * re-anchoring at :24-32 / :51-59); their estimates are NaN.  With mp->ld > R the three
 * planes are R-column windows of rows ld elements apart.
 * A flag byte of any nonzero value is a hit.  Slots of d_est / d_cells at or past
 * min(d_count[cpi*2], max_hits) are left untouched. */
typedef struct {
    int32_t extra_dots;      /* extraDots (2), 1..4: 2*extraDots+1 cells per spline */
    int32_t r_interp;        /* rInterpTimes (8), 1..64 */
    int32_t v_interp;        /* vInterpTimes (4), 1..64 */
    int32_t mtd0_num;        /* MTD_0_num: rows 1..M0+1 and V-M0+1..V are clutter-zeroed */
    int32_t beam_pos_num;    /* beamPosNum */
    double delta_r;          /* deltaR [m] */
    double delta_v;          /* deltaV [m/s] */
    double k_value;          /* kValues(freInd+1, beamPosNum+1) (angle_KvalueGen.m) */
    double beam_angle_step;  /* beamAngleStep [deg] (5) */
    double ele_comp;         /* eleAngleComp */
    double ele_sys_err;      /* eleAngleSysErr */
    int64_t ld;              /* row pitch of the planes in elements (0 = R): a column window of a
                                wider plane, e.g. DMX's short part (columns 0..61) or long part
                                (62..573, pass the planes + 62) measured separately as the
                                reference does (DMX_SignalProcessing_main_xzr.m:489-494) */
    int64_t cpi_stride;      /* elements between CPIs (0 = V * ld) */
} rsp_measure_params;

int rsp_motion_measure_dev(rsp_ctx* ctx, const float* d_sum, const float* d_diff, const uint8_t* d_flag,
                           int64_t V, int64_t R, int64_t batch, const rsp_measure_params* mp,
                           const double* d_r_scale, const double* d_v_scale, int64_t max_hits,
                           double* d_est, int32_t* d_cells /* nullable */, int32_t* d_count, void* stream);

/* The hit-list geometry a call would take (read-only; an addition within ABI 5): nothing is
 * launched and no buffer is touched.  d_flag is looked at for its alignment only (it is never
 * dereferenced; NULL is refused as the call refuses it).  Returns what rsp_motion_measure_dev's own
 * validation of V, R, batch and mp would return; ctx may be NULL (it only receives the message).
 * One workgroup of 1024 threads lists a CPI's hits.  A thread owns `cw` adjacent columns of one
 * of `slices` row slices; a pass covers groups * cw columns and `passes` passes cover R.  Slice s
 * owns rows min(V, s*rows) .. min(V, (s+1)*rows), and keeps one bit per q of its rows to find
 * its hits again.  wide (16-byte flag loads, cw = 16) needs R % 16 == 0, R >= 256, and the flag
 * address, the row pitch and the CPI stride all multiples of 16; everything else reads bytes
 * (cw = 1).  The two paths give the same bytes.
 * The same geometry, from the peak plane's address and the window's V, R, ld and cpi_stride,
 * governs the list rsp_condense_dev makes from its peak plane (the order of d_plots). */
typedef struct {
    int32_t wide;     /* 1: 16-byte flag loads */
    int32_t cw;       /* columns per thread: 16 or 1 */
    int32_t groups;   /* column groups per pass: a power of two, 16 (wide) / 64 (bytes) .. 1024 */
    int32_t slices;   /* row slices: 1024 / groups */
    int32_t rows;     /* rows per slice: ceil(V / slices) (of a band's rows where bands > 1) */
    int32_t q;        /* rows per bit of a thread's row mask: ceil(rows / 64) */
    int32_t passes;   /* ceil(R / (groups * cw)) */
    int32_t bands;    /* workgroups per CPI: 1 in the shipped library */
} rsp_measure_plan_t;
int rsp_measure_plan(rsp_ctx* ctx, const uint8_t* d_flag, int64_t V, int64_t R, int64_t batch,
                     const rsp_measure_params* mp, rsp_measure_plan_t* out);

/* ---- plot condensation: one peak cell per cluster of CFAR hits -------------------------- */
/* The reference scatters one estimate per CFAR hit (DMX_SignalProcessing_main_xzr.m:530-558); the
 * local-peak gates that would thin them are commented out (Function_CFAR1D_sub.m, _fixCells.m:60-83).
 * rsp_condense_dev labels the connected hits of each CPI's V x R flag window and keeps each
 * cluster's ("plot's") strongest cell.
 *
 * Adjacency: hits (v1, r1), (v2, r2) are adjacent when dv <= gap_v and |r1 - r2| <= gap_r, with
 * dv = |v1 - v2|, or min(|v1 - v2|, V - |v1 - v2|) with wrap_v (the Doppler axis is periodic: a
 * target at the folding velocity straddles rows 0 and V-1 of an fftshifted RDM).  gap 1, 1 is
 * 8-connectivity; 0, 0 makes every hit its own plot.  A plot is a connected component of the
 * transitive closure.  Hits never join across the window's column edges.
 * Peak: the plot's hit with the largest amplitude, compared as float32 values; on equal
 * amplitudes the first in MATLAB's find() order (the smallest r*V + v), the tie rule of
 * executeCFAR.m:69-70.  Amplitudes at flagged cells are magnitudes: where one is negative or NaN
 * the choice of peak is unspecified.
 *
 * d_amp: float32, d_flag: uint8 (nonzero = hit), d_peak: uint8, all [batch][V][ld] windows of the
 * same geometry (cp->ld, cp->cpi_stride).  Per CPI:
 *   d_peak   1 at each plot's peak cell, 0 at every other cell of the window: every cell of the
 *            window is written (the caller clears nothing; cells outside the window's columns
 *            are not touched), also when d_plots overflows.  rsp_motion_measure_dev takes it as
 *            its d_flag: hit i of that measurement is plot i.
 *   d_plots  int32 [batch][max_plots][8] or NULL: {peak_v, peak_r, n_cells, v_min, v_max, r_min,
 *            r_max, 0}, 0-based and relative to the window, ordered by the peak's find() order.
 *            v_min / v_max are the plain minimum and maximum of the row indices: a plot joined
 *            across the seam by wrap_v reports 0 and V-1.  Plots past max_plots are counted, not
 *            written, and the rest of d_plots is left untouched.
 *   d_count  int32 [batch][2] = {n_plots, n_hits}.
 * Every combination across threads is an integer atomic (min, max, add) whose result does not
 * depend on the order of arrival: two runs give the same bytes, and a CPI gives the same bytes
 * alone as inside a batch.
 * Memory: the context's grow-only condensation pool holds, per CPI of a chunk, 16 B per cell of
 * the window (an int32 label, a 64-bit peak key and an int32 hit-list slot, each touched at
 * flagged cells only) + 24 B x min(max_plots, V*R) + 16 B; 2048 x 512 with max_plots 4096:
 * 16.1 MiB per CPI, 4.0 GiB at batch 256.  The pool grows to batch x that and is capped at 8 GiB
 * (one CPI where a CPI needs more): a batch that needs more runs as consecutive chunks of
 * floor(8 GiB / bytes per CPI) CPIs on the stream (509 CPIs at 2048 x 512).
 * Asynchronous on `stream`; works on any context, the CFAR-only kind included. */
typedef struct {
    int32_t gap_v, gap_r;   /* 0..4 each */
    int32_t wrap_v;         /* 0/1; 1 needs V > 2*gap_v */
    int32_t reserved;       /* 0 */
    int64_t ld;             /* row pitch in elements (0 = R), as rsp_measure_params.ld */
    int64_t cpi_stride;     /* elements between CPIs (0 = V * ld) */
} rsp_condense_params;

int rsp_condense_dev(rsp_ctx* ctx, const float* d_amp, const uint8_t* d_flag, int64_t V, int64_t R,
                     int64_t batch, const rsp_condense_params* cp, uint8_t* d_peak,
                     int32_t max_plots, int32_t* d_plots /* nullable */, int32_t* d_count, void* stream);

/* ---- clutter map: detection in the zero-velocity band the chain blanks -------------------- */
/* fun_0v_pressing writes zeros over the Doppler rows round zero velocity, executeCFAR strips
 * rows 1..M0+1 and V-M0+1..V, and the DMX main zeroes rows 1:MTD_0_num+1 and
 * end-MTD_0_num+1:end: inside that band the chain flags nothing, a hovering target included.
 * rsp_cmap_dev is the classical MTD's answer: for each cell of the band's Doppler filters it
 * keeps a recursive average over CPIs (the "map") and flags a cell that stands over its own
 * history.  It is the one stage that carries state from call to call; the state (d_map, d_age)
 * is the caller's memory.
 *
 * Input: the pulse-compressed rows, d_pc complex64 [batch][beams][P][ld] (rsp_pc_dev's output).
 * Band amplitude of signed DFT bin q_k = q_lo + k, k < K = q_hi - q_lo + 1:
 *   a[b][k][r] = sum over beams of | sum_p win[p] * pc[p][r] * exp(-2 pi j q_k p / V) |
 * which is the value the MTD writes to the RDM row of bin q_k (row q_k mod V, or
 * (q_k + V/2) mod V of an fftshifted RDM) before that row is zeroed.  The table
 * win[p] * exp(...) is built in fp64 on the host, stored as fp32 and cached in the context by
 * (P, V, window, window_beta, q_lo, q_hi): the first call with a new key allocates and uploads
 * it synchronously, later calls only launch.  The sum over the pulses is an fp32 fmaf chain in
 * pulse order, or with a pulse split (rsp_cmap_plan_t.split = 4) four such chains over quarters
 * of the pulses added in quarter order.
 *
 * Map: the CPIs of a batch are consecutive in time and are applied in batch order, also when
 * several share a slot.  With s = d_slot[b] (0 when d_slot is NULL), m = map[s][k][r],
 * n = age[s], every operation a separate fp32 operation (nothing is contracted):
 *   flag = n >= max(warmup, 1) && a >= (float)T * m
 *   m'   = a                       when n == 0
 *   m'   = m                       when hold && flag
 *   m'   = m + (float)w * (a - m)  otherwise
 * and after the CPI's cells age[s] = n + 1, saturating at INT32_MAX.  A CPI whose slot is
 * negative (or >= slots) writes its band amplitudes and zero flags and touches no state.
 * Reset = zeroing d_age (the map needs no clearing: n == 0 overwrites it).
 * The fp32 map follows the exact recursion to about 2^-24 / w relative (each update rounds m
 * once and the recursion forgets an error at the rate w), so its error grows as 1 / w:
 * 2.4e-7 at w = 1/4, 4.8e-7 at w = 1/8, 6e-6 at w = 1/100.
 * No atomics and no floating-point combination whose order depends on scheduling: two runs give
 * the same bytes, and a sequence of CPIs gives the same map, age, band and flags in one batch as
 * in any split into consecutive calls.
 *
 * d_map float32 [slots][K][R], d_age int32 [slots], d_band float32 [batch][K][R] or NULL (the
 * amplitudes then pass through the context's grow-only pool, batch*K*R*4 bytes), d_flag uint8
 * [batch][K][R].  None may overlap another or d_pc.  Arguments are checked before the context
 * is looked at (RSP_ERR_ARG with a message).  Asynchronous on `stream`; works on any context,
 * the CFAR-only kind included. */
#define RSP_CMAP_MAX_BINS 64
typedef struct {
    int64_t P, V;            /* pulses; DFT length V >= P (zero-padded), V = 0 means P.  ANY P >= 2: a direct DFT has no radix limit */
    int32_t beams;           /* 1, or 2: amplitude = |X_L| + |X_R| as the DMX sum plane */
    int32_t window;          /* rsp_window */
    double  window_beta;
    int32_t q_lo, q_hi;      /* signed DFT bins q_lo..q_hi (q_lo <= 0 <= q_hi not required), K = q_hi-q_lo+1 <= 64, |q| < V/2 */
    int32_t warmup;          /* a slot flags nothing before it has absorbed max(warmup, 1) CPIs */
    int32_t hold;            /* 1: a flagged cell does not update its map value */
    double  T;               /* threshold factor */
    double  w;               /* 0 < w <= 1 */
    int64_t ld, cpi_stride;  /* row pitch (0 = R) and elements between CPIs (0 = beams*P*ld) of d_pc; overlapping CPIs allowed (window mode) */
} rsp_cmap_params;

int rsp_cmap_dev(rsp_ctx* ctx, const void* d_pc /* complex64 [batch][beams][P][ld] */, int64_t R, int64_t batch,
                 const rsp_cmap_params* mp, const int32_t* d_slot /* [batch]; NULL = slot 0; < 0: CPI updates nothing */,
                 int32_t slots, float* d_map /* [slots][K][R] */, int32_t* d_age /* [slots] */,
                 float* d_band /* [batch][K][R], nullable */, uint8_t* d_flag /* [batch][K][R] */, void* stream);

/* The band kernel instance a call takes (read-only; nothing is launched).  The K bins run in
 * `passes` groups of `bins_per_pass` (compile-time; bin k is accumulator k % bins_per_pass of pass
 * k / bins_per_pass, the table is padded with zero entries to kpad = passes * bins_per_pass).
 * vec: adjacent range columns per thread, 2 = 16-byte loads (R, ld and cpi_stride even), 1 =
 * 8-byte loads; a call whose d_pc is not 16-byte or d_band not 8-byte aligned takes vec = 1
 * whatever the plan says (same bytes out: a column's arithmetic does not depend on vec).
 * split: waves of a workgroup that share a column's pulses, 4 where R <= 1024 and P >= 256 (the
 * columns alone would not fill the part), else 1; it depends on R and P only, never on batch, so
 * a split of the batch cannot change a bit.  ctx may be NULL. */
typedef struct {
    int32_t K, kpad;
    int32_t bins_per_pass;   /* 4 (K <= 4) or 16 */
    int32_t passes;
    int32_t vec;             /* 1 or 2 */
    int32_t split;           /* 1 or 4 */
    int32_t threads;         /* per band workgroup: 64 * split */
    int32_t reserved;
    int64_t table_bytes;     /* the cached table: P * kpad * 8 */
    int64_t pool_bytes;      /* the context pool used when d_band == NULL: batch * K * R * 4 */
} rsp_cmap_plan_t;
int rsp_cmap_plan(rsp_ctx* ctx, int64_t R, int64_t batch, const rsp_cmap_params* mp, rsp_cmap_plan_t* out);

/* ---- Doppler line width per range column (ampConstrWidthEst.m) ---------------------------- */
/* widthDots = ampConstrWidthEst(specData, ampConstr, interpFlag, interpTimes) of
 * MatlabProcess_xuzerui/CFAR_WangCai, for every column of an amplitude plane that carries a hit:
 *   y = abs(fftshift(specData))                                  (the rotation by floor(V/2) when shift = 1)
 *   s = interp1(0:V-1, y, 0:1/interpTimes:V-1, 'spline')         (not-a-knot cubic, unit knots; s = y at interp = 1)
 *   M1 = max(s); the samples with 20*log10(s/M1) >= ampConstr; the last one's abscissa minus the first's.
 * A negative s/M1 makes MATLAB's log10 complex and >= compares real parts, so the test is
 * |s_i| >= 10^(amp_constr/20) * M1, which is how it is evaluated here (the level in fp64 on the
 * host, no logarithm on the device).  The figures (70, 71) and the commented-out walk outward from
 * the peak (:22-35) are not part of it.
 *
 * d_amp float32 and d_flag uint8 are [batch][V][ld] windows of R columns with the geometry of
 * rsp_motion_measure_dev and rsp_condense_dev.  A column is computed when any of its V flag bytes
 * inside the window is nonzero (d_flag == NULL: every column); the amplitudes of a column without
 * a hit are not read.  d_span int32 [batch][R][2]: a computed column's {first, last}, the 0-based
 * indices on the 1/interp grid (sample i lies at abscissa i / interp, i <= (V-1)*interp) of its
 * first and last sample at or above the level, so widthDots = (last - first) / interp; {-1, -1}
 * for a column that is not computed or whose M1 is not positive (an all-zero column: the
 * reference's 0/0 and empty set, width 0).  Every entry is written.  d_count int32 [batch]: the
 * columns computed.  Amplitudes are magnitudes; a NaN or Inf in a computed column leaves that
 * column's span unspecified.
 *
 * From the float32 inputs on the arithmetic is fp64: the second derivatives solve the (1, 4, 1)
 * rows by the Thomas algorithm (its two sweeps as parallel scans of affine maps)
 * and each interval is evaluated in the local power form.  The operation order differs from
 * MATLAB's, so a sample within rounding (a small multiple of 1e-16 of M1) of the level may fall
 * on the other side; away from such ties the integers are the reference's.  amp_constr = 0 is
 * refused: the level would coincide with the maximum itself, a tie in every column.
 * No floating-point operation depends on scheduling (the count is an integer sum): two runs give
 * the same bytes, and a CPI alone gives the bytes it gives inside a batch.
 * Limits: 4 <= V <= 2048, R >= 1, ld >= R.  Arguments are checked before the context is looked at
 * (RSP_ERR_ARG with a message).  Asynchronous on `stream`; works on any context, the CFAR-only
 * kind included; uses no context scratch. */
#define RSP_WIDTH_MIN_V 4
#define RSP_WIDTH_MAX_V 2048
typedef struct {
    double  amp_constr;   /* ampConstr [dB]: -200 <= amp_constr < 0 */
    int32_t interp;       /* interpTimes 1..64; 1 = interpFlag 0 */
    int32_t shift;        /* 1: fftshift each column first, as the .m does (the DMX planes, which carry no shift);
                             0: the plane is already centred (the v2 / legacy RDM) */
    int64_t ld;           /* row pitch in elements (0 = R), as rsp_measure_params.ld */
    int64_t cpi_stride;   /* elements between CPIs (0 = V * ld) */
} rsp_width_params;

int rsp_spec_width_dev(rsp_ctx* ctx, const float* d_amp, const uint8_t* d_flag /* nullable */,
                       int64_t V, int64_t R, int64_t batch, const rsp_width_params* wp,
                       int32_t* d_span, int32_t* d_count, void* stream);

/* ---- ordered-statistic CFAR: a second detector beside the GO/SO cell-averaging one --------- */
/* executeCFAR.m with one substitution: the noise estimate of a reference window is its k-th
 * smallest cell, not its mean.  A second target inside a reference window raises the mean and
 * masks its neighbour; it moves the k-th smallest cell only when k cells or more are occupied.
 * Everything else is rsp_cfar_dev's: the row band [M0 + 1, V - M0), the column segments (columns
 * outside every segment are flagged 0), the rows of the zero_v_div band read as 0, the Doppler test
 * on every band cell of every in-segment column (flagV), and with rFlag = 1 the range test on r-1,
 * r, r+1 of every Doppler hit, confined to the hit's segment, the first maximum among the passing
 * cells flagged (rFlag = 0: flag = flagV).
 *
 * For cell y of a line z whose valid part is [lo, hi) (a column's band rows; a band row's segment):
 * L = [y-save-ref, y-save-1], Rt = [y+save+1, y+save+ref]; a side that leaves [lo, hi) is replaced
 * by the other side (Function_CFAR1D_sub.m:30-39).
 *   per side (union = 0, 1 <= k <= ref): a, b = the k-th smallest of z[L], z[Rt];
 *                                        w = max(a, b) (method 0, GO) or min(a, b) (method 1, SO);
 *   union    (union = 1, 1 <= k <= 2*ref, method ignored): w = the k-th smallest of the 2*ref
 *                                        values of both sides as a multiset (at a one-sided cell the
 *                                        valid side's values count twice).
 * The cell passes iff z[y] >= fl32((float)T * w): one fp32 multiply, rounded to nearest.  T
 * multiplies the order statistic itself; it is not divided by ref.
 * Multiplication by a positive constant is monotone in IEEE arithmetic, so the test holds exactly
 * when at least k window cells satisfy fl32(T * z_i) <= z[y]; with the side counts cl, cr (a missing
 * side takes the other's count): GO cl >= k and cr >= k, SO cl >= k or cr >= k, union cl + cr >= k.
 * The kernels count; they neither sort nor select, and the flags are bit-exact
 * against a sorted restatement in fp32.  Inputs are magnitudes (finite, >= 0); a NaN leaves the
 * cells whose windows contain it unspecified.
 *
 * d_rdm float32, d_flag and d_flagV (nullable) uint8 are [batch][V][ld] windows of R columns with
 * the geometry of rsp_condense_dev / rsp_spec_width_dev.  Every byte of the window in d_flag (and
 * d_flagV) is written; nothing outside the window is read or written.  cfar keeps its field
 * meanings; the checks are rsp_cfar_dev's with the same codes, and further T finite and > 0 and k
 * in range for its form (RSP_ERR_ARG); ref > RSP_OS_MAX_REF per side or V > RSP_OS_MAX_V:
 * RSP_ERR_UNSUPPORTED (as is rsp_cfar_dev's own limit, a range guard + ref over 30 cells).  Arguments
 * are checked before the context is looked at.  With rFlag = 1 and d_flagV == NULL the Doppler flags go to the context's scratch.
 * No atomics; a flag byte is written once, by one thread: two runs give the same bytes, and a CPI
 * alone gives the bytes it gives inside a batch.  Asynchronous on `stream`; works on any context,
 * the CFAR-only kind included.  Timed under rsp_profile as RSP_K_OS_V / RSP_K_OS_R. */
#define RSP_OS_MAX_REF 32
#define RSP_OS_MAX_V 4096
typedef struct {
    int32_t kV, kR;          /* 1-based rank of the Doppler / range test */
    int32_t unionV, unionR;  /* 0: per side, then methodV/methodR (0 GO, 1 SO); 1: both sides as one set */
    int64_t ld;              /* row pitch in elements (0 = R), as rsp_width_params.ld */
    int64_t cpi_stride;      /* elements between CPIs (0 = V * ld) */
} rsp_os_params;

int rsp_os_cfar_dev(rsp_ctx* ctx, const float* d_rdm, int64_t V, int64_t R, int64_t batch,
                    const rsp_cfar_params* cfar, const rsp_os_params* os,
                    uint8_t* d_flag, uint8_t* d_flagV /* nullable */, void* stream);

/* The launches that call would make (read-only; nothing is launched, no buffer is touched), from the
 * launchers' own host functions.  The Doppler kernel is one piece of code whose tile of
 * 2^v_tile_log2 columns x V rows is sized by V alone (1..6 for V <= RSP_OS_MAX_V); the range stage
 * is absent with rFlag = 0, where the Doppler kernel stores flag itself.  Returns what the call's
 * validation would return. */
enum { RSP_OS_R_NONE = 0,      /* rFlag == 0: the Doppler kernel writes flag = flagV */
       RSP_OS_R_GATHER = 1 };  /* one workgroup per tile of a row; a tile without a Doppler hit in reach
                                  stores zeros and leaves */
typedef struct {
    int32_t v_tile_log2;   /* log2 of the Doppler tile's columns */
    int32_t v_pitch;       /* floats between the tile's columns in LDS */
    int32_t r_stage;       /* RSP_OS_R_* */
    int32_t r_tile;        /* columns per range workgroup (0 with RSP_OS_R_NONE) */
    int32_t r_tiles;       /* range workgroups per row */
    int32_t r_halo;        /* columns staged on each side of a range tile: guard + ref + 2 */
    int32_t scratch_flagV; /* 1: flagV goes to the context's scratch (rFlag = 1, no d_flagV) */
    int32_t reserved;      /* 0 */
} rsp_os_plan_t;
int rsp_os_cfar_plan(rsp_ctx* ctx, int64_t V, int64_t R, int64_t batch, const rsp_cfar_params* cfar,
                     const rsp_os_params* os, int32_t with_flagV, rsp_os_plan_t* out);

/* ---- tracking: the plots of successive CPIs joined into tracks ----------------------------- */
/* DMX_SignalProcessing_main_xzr.m plots each frame's {rEst, vEst, eleAngleEst} against the frame
 * number and GPS truth (:530-601); the reference ships no stage that says which estimates of
 * successive frames are one target.  rsp_track_dev is that stage: gated nearest-neighbour
 * association with fixed smoothing gains and M-of-N confirmation, behind rsp_motion_measure_dev
 * and on its outputs as they stand.  Like the clutter map it carries state from call to call, and
 * the state is the caller's memory.
 *
 * Input: d_est double [batch][max_hits][3] = {r, v, ele} and d_count int32 [batch][2]; the
 * n = min(d_count[2b], max_hits) first plots of CPI b are read.  A plot is valid when neither its
 * r nor its v is NaN.
 * State: per slot max_tracks entries, d_state_f double [slots][max_tracks][4] = {r, v, ele, 0} and
 * d_state_i int32 [slots][max_tracks][8] = {id, status, hist, misses, hits, age, last_plot, 0};
 * status 0 free, 1 tentative, 2 confirmed; hist the hit history, bit 0 the latest CPI; d_meta
 * int32 [slots][2] = {next_id, cpis}.  A free entry is all zero bytes; reset = zeroing the three
 * arrays.
 * Slots: s = d_slot[b] (0 when d_slot is NULL).  The CPIs of a batch are consecutive in time and
 * are applied in batch order, also when several share a slot.  A CPI whose slot is negative or
 * >= slots touches no state; its d_assign row is -1 for an invalid plot and 0 otherwise, its
 * snapshot all zero bytes and its d_tcount row {0, 0, 0, 0, 0, n_valid, 0, 0}.
 *
 * One CPI, with h = d_dt[b] (tp->dt when d_dt is NULL), wr = 1/(gate_r*gate_r) and
 * wv = 1/(gate_v*gate_v) in fp64 on the host; every floating-point operation below is a separate
 * fp64 operation in the order written (nothing is contracted):
 *   1 predict    every live track: rp = r + ((rate_sign*v)*h), vp = v.
 *   2 gate       (t, j) is a candidate when |r_j - rp| <= gate_r and |v_j - vp| <= gate_v, with
 *                dr = r_j - rp, dv = v_j - vp, cost c = ((dr*dr)*wr) + ((dv*dv)*wv) and key
 *                (status == 2 ? 0 : 1, c, t, j), ordered lexicographically; t is the entry index.
 *   3 associate  the candidates in ascending key order, skipping one whose track or plot is taken.
 *   4 update     matched: r = rp + alpha_r*(r_j - rp), v = vp + alpha_v*(v_j - vp); ele unchanged
 *                when ele_j is NaN, ele_j when the track's is NaN, else ele + alpha_e*(ele_j - ele);
 *                hist = (hist<<1)|1, misses = 0, hits += 1, last_plot = j.
 *                unmatched: r = rp, v = vp, hist <<= 1, misses += 1, last_plot = -1.
 *                both: age += 1.
 *   5 confirm    a tentative track with popcount(hist & mask_N) >= M becomes confirmed; then a
 *     and drop   track that is still tentative is deleted when misses >= drop_tentative or
 *                age >= N, a confirmed one when misses >= drop_confirmed.  A deleted entry is zeroed.
 *   6 start      the valid unmatched plots, in plot order, take the free entries in index order
 *                (those freed in step 5 included): {r_j, v_j, ele_j}, id = ++next_id (ids start
 *                at 1), tentative (confirmed when M = 1), hist = 1, hits = 1, age = 1, misses = 0,
 *                last_plot = j.  Plots left without an entry are counted.
 *                d_assign int32 [batch][max_hits]: the id the plot updated or started, 0 for a
 *                valid plot that did neither, -1 for an invalid one, 0 at and past n.
 *   7 record     cpis += 1; d_snap_f / d_snap_i [batch][max_tracks][4] / [8] (both or neither): the
 *                slot's whole state after the CPI; d_tcount int32 [batch][8] = {live, confirmed,
 *                started, dropped, not_started, n_valid, matched, 0}.
 * One workgroup per slot walks its CPIs inside one launch, the table in LDS; the matching runs as
 * rounds of mutual-best pairs, which the strict total order of the keys makes equal to step 3.
 * The only atomics are integer minima and counts, whose results do not depend on arrival order,
 * and no floating-point value is combined across threads: two runs give the same bytes, and a
 * sequence of CPIs gives the same state and outputs in one batch as in any split into
 * consecutive calls.
 * Limits: 56*max_tracks + 32*max_hits <= 163328 bytes of LDS (RSP_ERR_UNSUPPORTED otherwise):
 * max_hits <= 4656 at max_tracks 256, <= 3312 at 1024.  No buffer may overlap another.  Arguments
 * are checked before the context is looked at (RSP_ERR_ARG with a message).  Asynchronous on
 * `stream`; works on any context, the CFAR-only kind included; uses no context scratch. */
#define RSP_TRACK_MAX_TRACKS 1024
typedef struct {
    int32_t max_tracks;        /* 1..1024 track entries per slot */
    int32_t confirm_m, confirm_n;  /* 1 <= M <= N <= 32 */
    int32_t drop_tentative;    /* >= 1: consecutive misses that delete a tentative track */
    int32_t drop_confirmed;    /* >= 1: consecutive misses that delete a confirmed track */
    int32_t reserved;          /* 0 */
    double  dt;                /* seconds between consecutive CPIs of a slot (frame time P*prt, :571); > 0 */
    double  rate_sign;         /* +1 or -1: range moves by rate_sign * v * dt */
    double  gate_r, gate_v;    /* > 0, in the units of rEst / vEst */
    double  alpha_r, alpha_v, alpha_e;  /* smoothing gains, each in (0, 1] */
} rsp_track_params;

int rsp_track_dev(rsp_ctx* ctx, const double* d_est /* [batch][max_hits][3] */,
                  const int32_t* d_count /* [batch][2] */, int64_t max_hits, int64_t batch,
                  const rsp_track_params* tp, const int32_t* d_slot /* [batch] or NULL */,
                  const double* d_dt /* [batch] or NULL */, int32_t slots,
                  double* d_state_f /* [slots][max_tracks][4] */, int32_t* d_state_i /* [slots][max_tracks][8] */,
                  int32_t* d_meta /* [slots][2] */, int32_t* d_assign /* [batch][max_hits] */,
                  double* d_snap_f /* [batch][max_tracks][4] or NULL */, int32_t* d_snap_i /* same, [8] */,
                  int32_t* d_tcount /* [batch][8] */, void* stream);

/* ---- post-detection integration over the CPIs of a dwell ----------------------------------- */
/* Every detector here decides on one CPI alone; only rsp_track_dev looks across CPIs, after hard
 * decisions.  A target below the threshold in every CPI of a dwell is lost.  These two calls are the
 * classical answer, between the MTD and the CFAR (the reference ships no such stage):
 *   rsp_integrate_dev  video (non-coherent) integration: the amplitude planes of the last n CPIs are
 *                      summed before the CFAR;
 *   rsp_binint_dev     binary (M-of-N) integration: the flag planes of the last n CPIs are counted
 *                      after the CFAR.
 * The RDM orders the cells by velocity, so Doppler row v has a known range walk per CPI (a DMX frame
 * is 80 ms and a range cell 12 m: 150 m/s is one cell per CPI); each past plane is shifted row by row
 * before it is added, and the target piles up in one cell instead of smearing over n.
 *
 * d_in, d_out: [batch][V][ld] windows of R columns (float32 / uint8), geometry as rsp_os_params'.
 * Like the clutter map and the tracker the stage carries state from call to call in the caller's
 * memory: d_hist [slots][n-1][V][R], a ring of the last n-1 input planes of each slot, stored dense
 * (window columns only), and d_meta int32 [slots][2] = {cpis, 0}.
 *
 * CPI b of a batch, in batch order.  s = d_slot[b] (0 when d_slot is NULL).
 *   s < 0 or s >= slots: the CPI touches no state, n_eff = 1: it is integrated as the first CPI of a
 *     slot would be.
 *   otherwise k = d_meta[2s], the CPIs the slot has seen (a negative count reads as 0), and
 *     n_eff = min(n, k + 1).  x_0 is the CPI itself, x_i (1 <= i < n_eff) the plane i CPIs back on
 *     the slot.
 *   A target that stood at column c of row v i CPIs ago stands at c + d_shift[(i-1)*V + v] now (0 when
 *   d_shift is NULL): the term of x_i at (v, r) is x_i[v][r - shift].  A source column outside [0, R)
 *   gives +0.0f (no hit in the binary form): nothing wraps, nothing crosses the window's column edges,
 *   any int32 shift is legal.
 *   sum     acc = x_0[v][r]; acc = acc + term_i for i = 1 .. n_eff-1 in that order, every addition a
 *           separate fp32 add; an out-of-window term is added as +0.0f, not skipped; NaN and Inf
 *           propagate as IEEE says.  d_out[v][r] = acc.  The result is a sum, not a mean: the first
 *           n-1 CPIs of a slot come out at a smaller scale than the later ones.  Every consumer here
 *           (the CFARs, the measurement, the width) compares ratios inside one plane, so that scale
 *           does not matter to them; a caller that wants a mean divides by d_neff.
 *   binary  cnt = (x_0[v][r] != 0) plus one for each i >= 1 for which any of the columns
 *           r - shift - spread .. r - shift + spread that lie inside the window is nonzero in x_i[v];
 *           d_out[v][r] = cnt >= m ? 1 : 0.  Strict: with m > 1 a slot flags nothing before its m-th CPI.
 *   state   d_neff[b] = n_eff.  In-range slot: with n > 1 the input plane becomes ring entry
 *           k mod (n-1) of the slot; then d_meta[2s] = k + 1 (also with n = 1, which keeps no planes).
 *           Ring entries that are not overwritten keep their bytes, d_meta[2s+1] is not touched.
 *           Reset = zeroing d_meta; d_hist need not be cleared, n_eff never reaches an entry that was
 *           not written since the reset.
 * d_out, d_neff, d_hist and d_meta after a sequence of CPIs are the same bytes in one batch as in any
 * split into consecutive calls, and the same from run to run (no atomics, nothing combined across
 * threads).  Only window columns of d_out are written.
 *
 * Refused with RSP_ERR_ARG and a message, before the context is looked at: a NULL params, d_in,
 * d_meta or d_out, d_hist NULL with n > 1; n outside 1..16; sum form with m or spread nonzero,
 * binary form with m outside 1..n or spread outside 0..2; reserved != 0; ld < R or a CPI stride
 * below a plane; slots outside 1..65535; misaligned pointers; d_out overlapping d_in or d_hist (in
 * place is not allowed: later CPIs of a batch read earlier input planes), d_in overlapping d_hist.
 * Asynchronous on `stream`; works on any context, the CFAR-only kind included.  Three launches
 * (plan, integrate, ring update); nothing is allocated, freed or copied synchronously
 * in the launch path except growth of the context's plan table (batch * (n + 3) ints, grow-only). */
#define RSP_INTEG_MAX_N 16
typedef struct {
    int32_t n;          /* 1..16: the CPI itself and the n-1 before it on its slot */
    int32_t m;          /* binary form: 1..n; sum form: 0 */
    int32_t spread;     /* binary form: 0..2 columns; sum form: 0 */
    int32_t reserved;   /* 0 */
    int64_t ld;         /* row pitch of d_in and d_out in elements (0 = R) */
    int64_t cpi_stride; /* elements between CPIs of d_in and d_out (0 = V * ld) */
} rsp_integ_params;

int rsp_integrate_dev(rsp_ctx* ctx, const float* d_in, int64_t V, int64_t R, int64_t batch,
                      const rsp_integ_params* ip, const int32_t* d_shift /* [n-1][V] or NULL */,
                      const int32_t* d_slot /* [batch] or NULL */, int32_t slots,
                      float* d_hist /* [slots][n-1][V][R]; NULL only when n == 1 */,
                      int32_t* d_meta /* [slots][2] = {cpis, 0} */,
                      float* d_out, int32_t* d_neff /* [batch] or NULL */, void* stream);

int rsp_binint_dev(rsp_ctx* ctx, const uint8_t* d_in, int64_t V, int64_t R, int64_t batch,
                   const rsp_integ_params* ip, const int32_t* d_shift, const int32_t* d_slot, int32_t slots,
                   uint8_t* d_hist, int32_t* d_meta, uint8_t* d_out, int32_t* d_neff, void* stream);

/* ---- stacked beams: the hits fused per cell, elevation from the beam amplitudes ------------- */
/* The v2 capture forms a stack of elevation beams, and rsp_window_pc_mtd_cfar_dev gives one RDM and
 * one flag plane per beam.  A target is flagged in two or three neighbouring beams at the same
 * (v, r), or in all of them through sidelobes; the reference stops there
 * (main_produce_dataset_win_xzr_v2.m:146-162 saves the planes).  These two calls merge the flags per
 * cell, say which beam the target sits in and estimate its elevation from the amplitudes of that
 * beam and its neighbours: rsp_beam_fuse_dev's d_famp / d_fflag go to rsp_condense_dev and
 * rsp_motion_measure_dev as they stand (d_famp as both the sum and the difference plane), and
 * rsp_beam_elev_dev writes the third estimate of that measurement, which rsp_track_dev reads.
 *
 * d_amp float32, d_flag uint8: `beams` planes per CPI, each V rows of R columns; cell (b, k, v, r) is
 * element b*cpi_stride + k*beam_stride + v*ld + r.  The three strides serve [batch][beams][V][ld]
 * (the defaults) and rsp_window_pc_mtd_cfar_dev's [beams][batch][V][R] (beam_stride = batch*V*R,
 * cpi_stride = V*R).  Every output is dense [batch][V][R].
 *
 * rsp_beam_fuse_dev, per cell (b, v, r), with a_k the float32 amplitude of beam k and f_k its flag
 * byte (any nonzero value is a hit):
 *   cnt      the number of k with f_k != 0; the cell is a fused hit when cnt >= min_beams.
 *   d_fcnt   uint8, nullable: cnt.
 *   d_fflag  uint8: 1 at a fused hit, otherwise 0.
 *   d_fbeam  uint8: at a fused hit the flagged beam with the largest amplitude, compared as float32
 *            with `>` in beam order (the first of equal amplitudes wins); elsewhere 255.
 *   d_famp   float32, nullable: m after m = a_0; for k = 1 ..: if (a_k > m) m = a_k -- over all beams,
 *            flagged or not, at every cell.  With a NaN amplitude d_famp and d_fbeam are
 *            unspecified, as the peak of rsp_condense_dev is.
 * Every cell of every output is written once, by one thread; the caller clears nothing.  No atomics,
 * no LDS, nothing combined across threads: two runs give the same bytes, and a CPI gives the same
 * bytes alone as inside a batch.  A thread owns four consecutive columns of one row of one CPI and
 * loads them with one 16-byte amplitude load (4-byte aligned) and one 4-byte flag load per beam; it
 * takes its cells one by one where they run past the row end or where a flag or byte-output address
 * of its four cells is not 4-byte aligned (odd R, ld, strides or bases).  Both ways give the same
 * bytes.  One launch per 2^30 workgroups, asynchronous on `stream`; nothing is allocated or copied.
 *
 * rsp_beam_elev_dev, one thread per listed hit.  d_cells int32 [batch][max_hits][2] = (row, col) and
 * d_count int32 [batch][2] are what rsp_motion_measure_dev writes, on d_famp with d_fflag or with a
 * condensed peak plane.  Hit i < min(d_count[cpi*2], max_hits) of a CPI gets
 * d_el[(cpi*max_hits + i) * el_stride] (float64; el_stride = 3 and d_el = d_est + 2 is the
 * measurement's est[..][2]) and, with d_hb (int32 [batch][max_hits][4]), {peak beam k, flagged beams
 * at the cell, lower beam used, upper beam used}; the last two are k-1 and k+1 where the elevation
 * came from the three beams and -1, -1 where it is x_k or NaN, and the first is -1 where k is 255.
 * Entries at or past that count are left untouched, as is everything between the d_el entries.
 * With k = d_fbeam at the cell (read as 255 when it is >= beams, or when the cell lies outside
 * V x R), x_i = beam_el[i] and the amplitudes widened to double:
 *   1. k is 255: NaN.
 *   2. law == 0, or k is the first or the last beam: x_k.
 *   3. law == 1: w_i = a_i * a_i for i = k-1, k, k+1 (-, 0, +);
 *      el = ((w_- x_- + w_0 x_0) + w_+ x_+) / ((w_- + w_0) + w_+); x_k where the denominator is zero
 *      or not finite.
 *   4. law == 2: x_k where any of the three amplitudes is <= 0 or not finite.  Otherwise
 *      y_i = log(a_i), dm = x_0 - x_-, dp = x_0 - x_+, A = y_0 - y_+, B = y_0 - y_-,
 *      den = dm*A - dp*B, xv = x_0 - 0.5 * (dm*dm*A - dp*dp*B) / den; x_k where
 *      den * (x_+ - x_-) <= 0 (flat or convex) or xv is not finite; otherwise xv clamped to
 *      [min(x_-, x_+), max(x_-, x_+)].
 * For Gaussian beams of one width on any spacing log a is a parabola in the angle, and law 2 is exact
 * up to rounding.  All fp64, contraction off, in exactly this order (csrc/rsp_fuse_math.h).
 *
 * Refused with RSP_ERR_ARG and a message, before the context is looked at: a NULL params, input or
 * required output; beams outside 2..32, min_beams outside 1..beams, law outside 0..2, reserved != 0;
 * a bad shape; ld < R; strides under which the address ranges ((V-1)*ld + R elements each) of two
 * different (CPI, beam) planes overlap -- the beams of a CPI must lie inside its cpi_stride, or the
 * CPIs of a beam inside its beam_stride; non-finite or not strictly monotonic centres; misaligned
 * float, int or double pointers; an output of rsp_beam_fuse_dev that overlaps an input or another
 * output; and for
 * rsp_beam_elev_dev max_hits < 0, el_stride < 1 or more than 2^31 - 1 blocks of 256 hits.
 * Both work on any context, the CFAR-only kind included. */
#define RSP_FUSE_MAX_BEAMS 32
typedef struct {
    int32_t beams;          /* 2..32 */
    int32_t min_beams;      /* 1..beams: flagged beams a cell needs to become a fused hit */
    int32_t law;            /* 0 centre of the peak beam, 1 power centroid of three beams, 2 log-parabola */
    int32_t reserved;       /* 0 */
    int64_t ld;             /* row pitch of the input planes in elements (0 = R) */
    int64_t beam_stride;    /* elements between the beams' planes of one CPI (0 = V*ld) */
    int64_t cpi_stride;     /* elements between CPIs (0 = beams*V*ld) */
    double  beam_el[32];    /* beam centres [deg], strictly monotonic over the first `beams` */
} rsp_fuse_params;

int rsp_beam_fuse_dev(rsp_ctx* ctx, const float* d_amp, const uint8_t* d_flag, int64_t V, int64_t R,
                      int64_t batch, const rsp_fuse_params* fp, uint8_t* d_fflag, uint8_t* d_fbeam,
                      float* d_famp /* nullable */, uint8_t* d_fcnt /* nullable */, void* stream);

int rsp_beam_elev_dev(rsp_ctx* ctx, const float* d_amp, const uint8_t* d_flag, const uint8_t* d_fbeam,
                      int64_t V, int64_t R, int64_t batch, const rsp_fuse_params* fp,
                      const int32_t* d_cells /* [batch][max_hits][2], (row, col) */,
                      const int32_t* d_count /* [batch][2] */, int64_t max_hits,
                      double* d_el, int64_t el_stride, int32_t* d_hb /* nullable, [batch][max_hits][4] */,
                      void* stream);

/* ---- detection scoring against truth (main_cfar.m's evaluation functions) ---------------- */
/* The four local functions at the end of MatlabProcess_xuzerui/CFAR_WangCai/main_cfar.m, the
 * reason for its `for T=[5]` threshold loop (:40), over a device-resident batch of flag matrices:
 *   fa    = fun_frame_fa(cfarFlag, R_True, V_True, R_True_index, V_True_index)        (:163-175)
 *   drate = fun_drate(cfarFlag_all, R, V, r_axis, v_axis, frameRInds)                 (:177-206)
 *   acc   = fun_accuracy(cfarFlag_all, R, V, r_axis, v_axis, frameRInds)              (:208-234)
 *   pof   = fun_PCF(cfarFlag_all, R, V, r_axis, v_axis, frameRInds, MTD_data_all)     (:236-279)
 * Every one of them reduces a whole V x R flag matrix (fun_PCF: and the RDM) to a few integers
 * before any arithmetic.  rsp_score_dev computes those integers on the GPU, one 8-int record per
 * CPI; rsp_score_summary turns the records into the reference's numbers on the host, in its
 * operation order.  Only batch x 8 ints cross PCIe.
 *
 * d_flag: uint8 [batch][V][ld] with values 0/1 (the chain's d_flag), d_rdm: float32 of the same
 * geometry or NULL (no fun_PCF peak search), d_truth: int32 [batch][3] = {v_idx, r_idx, valid},
 * the truth's nearest axis bins, 0-based (MATLAB's V_True_index - 1, R_True_index - 1; :183-184
 * take the first bin of a tie), and whether the truth passes the gate
 * abs(V)>3 && abs(V)<20 && R>400 && R<2000 (:165, :186, :217, :246).  With sp->ld > R (and
 * sp->cpi_stride) the matrices are row / column windows of larger planes -- clip.m:12's rows
 * 691:845 of a 1536-row RDM are a pointer offset, not a copy.
 *
 * d_rec: int32 [batch][8] per CPI (fields 1..7 are 0 for a truth that is not valid):
 *   [0] n_flags     sum of all V x R flags
 *   [1] n_box       flags in rows v_idx-hv..v_idx+hv, columns r_idx-hr..r_idx+hr (:167, :188, :219),
 *                   the box clipped to the matrix
 *   [2] box_status  bit 0: the box leaves the matrix on the low side (an index error in all four
 *                   functions); bit 1: on the high side (an index error for the reads of
 *                   fun_drate / fun_accuracy; fun_frame_fa's assignment there grows its copy,
 *                   whose sum is unchanged, while m, n were taken before: no error)
 *   [3] n_pcf       flags in fun_PCF's box: +-n_cell around the truth after the if / elseif chain
 *                   of :248-258, which clips at most ONE side (the first that applies of: rows
 *                   below 1, rows above v_lim, columns below 1, columns above r_lim); 0 when that
 *                   box is an index error
 *   [4] pcf_status  bit 0: a non-empty range of that box still leaves the matrix (MATLAB stops)
 *   [5] n_peak      cells of the WHOLE matrix equal to the maximum of the RDM over the box
 *                   ([v_ind, r_ind] = find(local_max == MTD_data), :262, searches everything);
 *                   computed when n_pcf > 0 and d_rdm != NULL, otherwise 0.  NaN cells never match.
 *   [6] peak_v, [7] peak_r   0-based cell of the first match in find() order (smallest r*V + v)
 * Two or more matches make dv a vector and dv^2 a MATLAB error (:265): n_peak tells.
 * The records are combined from per-workgroup partial results with integer adds and an integer
 * minimum only, so they do not depend on scheduling.
 *
 * Quirks of the reference that are kept, not fixed:
 *   - `for i=1:length(cfarFlag_all)` (:179, :210, :238) is the LARGEST dimension of the 3-D array,
 *     the frame count only when there are more frames than rows and columns.  Here the loop
 *     runs over the batch.
 *   - fun_accuracy counts a frame without a valid truth when it holds ANY flag (:224-227).
 * Works on any context, the CFAR-only kind included; needs no per-context scratch (the partial
 * results accumulate in d_rec itself). */
typedef struct {
    int32_t hv, hr;          /* half height / width of the detection box (3, 7) */
    int32_t n_cell;          /* fun_PCF's n_cell (20) */
    int32_t v_lim, r_lim;    /* the limits fun_PCF's elseif chain compares with (155, 288: the
                                clipped dataset's size, hard-coded at :250-255); not assumed to be V, R */
    int32_t reserved;        /* 0 */
    int64_t ld;              /* row pitch of the planes in elements (0 = R) */
    int64_t cpi_stride;      /* elements between CPIs (0 = V * ld) */
} rsp_score_params;

enum { RSP_SCORE_FA = 0, RSP_SCORE_DRATE = 1, RSP_SCORE_ACC = 2, RSP_SCORE_PCF = 3 };

typedef struct {
    double drate;              /* fun_drate: #(t>0) / #(valid); 0/0 = NaN as in MATLAB */
    double acc;                /* fun_accuracy: count / batch */
    double pof;                /* fun_PCF: mean of the scored frames' pof; NaN when none scored */
    int64_t n_valid;           /* truths that pass the gate */
    int64_t n_scored;          /* frames in fun_PCF's pof_list */
    int64_t n_index_error[4];  /* CPIs at which the reference stops with an index error, by
                                  function (RSP_SCORE_*); they contribute nothing to that
                                  function's number (fa[i] = NaN) */
    int64_t n_multi_peak;      /* valid CPIs with n_peak > 1: fun_PCF stops at dv^2; left out of pof */
} rsp_score_result;

/* Asynchronous on `stream`. */
int rsp_score_dev(rsp_ctx* ctx, const uint8_t* d_flag, const float* d_rdm /* nullable */, int64_t V,
                  int64_t R, int64_t batch, const rsp_score_params* sp, const int32_t* d_truth,
                  int32_t* d_rec, void* stream);
/* Host only (no GPU, no context): rec / truth are host copies of d_rec / d_truth.  fa[i]
 * (nullable) = fun_frame_fa of CPI i; out = the batch's fun_drate, fun_accuracy, fun_PCF
 * (dv_base = 1/0.2719, dr_base = 30/6; pof = 1 - l/l_base below l_base, exp(1 - l/l_base) - 1
 * from there, :264-271) and the counters.  A CPI with n_pcf > 0 and n_peak == 0 (no RDM was
 * given) is not scored.  Returns RSP_ERR_ARG for a NULL rec / truth / sp / out. */
int rsp_score_summary(const int32_t* rec, const int32_t* truth, int64_t batch, int64_t V, int64_t R,
                      const rsp_score_params* sp, double* fa /* [batch], nullable */,
                      rsp_score_result* out);

/* ---- echo pre-filters ---------------------------------------------------- */
/* iSTC and MTI on a device-resident echo batch, complex64 [batch][P][R] (row = pulse, the
 * chain's ROWMAJOR layout), before pulse compression:
 *   d_gain != NULL: out(m, n) *= d_gain[n], the linear gain 10^(stc(n)/20) of
 *       [stc, eoch_iSTC] = fun_iSTC(echo)            (MTD/fun_iSTC.m:12-15; the caller reads
 *       the stc curve and zero-pads it to R as :8-9 do -- rsp/prefilter.py istc_gain);
 *   mti_lag > 0: out(m, :) = x(m+lag, :) - x(m, :) for m < P-lag, 0 for the last lag rows,
 *       MTI_Out = fun_Process_MTI(ProSiganl)          (MTD/fun_Process_MTI.m:9,20-22; lag 30).
 * Both: the MTI difference first, then the gain (the two commute up to fp32 rounding).
 * R must be even and d_in / d_out 16-byte aligned; d_out == d_in is allowed only without MTI. */
int rsp_prefilter_dev(rsp_ctx* ctx, const void* d_in, void* d_out, int64_t P, int64_t R, int64_t batch,
                      const float* d_gain /* nullable, [R] */, int32_t mti_lag, void* stream);

/* The same pre-filters fused into the context's chain (every rsp_pc_mtd*, rsp_run*, window
 * entry point after this call), with no pass of their own over the echo:
 *   gain != NULL (host, [R] linear gains as above): applied to each echo sample as pulse
 *       compression loads it (needs the per-segment PC kernels -- the v2, dmx and legacy
 *       presets; RSP_ERR_UNSUPPORTED otherwise);
 *   mti_lag > 0: applied to the pulse-compressed rows as the MTD loads them -- pulse
 *       compression is linear per row, so PC(x(m+lag) - x(m)) = PC(x(m+lag)) - PC(x(m)) --
 *       over the pulses of each CPI (each window in window mode), zero for its last lag rows.
 * gain == NULL and mti_lag == 0 switch the fused pre-filters off.
 * rsp_pc_dev (pulse compression alone) applies the gain but not MTI, which lives in the MTD
 * stage: its rows are PC(gain .* x). */
int rsp_set_prefilter(rsp_ctx* ctx, const float* gain /* nullable, host [R] */, int32_t mti_lag);

/* ---- target injection at a set SCR (fun_SCR / fun_add_clutter) ---------------------------- */
/* The target-injection step of MatlabProcess_xuzerui/main.m:183-194, which makes the truth R, V
 * that main_cfar.m's evaluation functions (above) score against, on a device-resident batch of
 * complex64 [batch][P][R] echoes (row = pulse):
 *   Echo_simu_STC = fun_SCR(prtNum, Echo_simu, echoData_Frame_0, SCR)      (fun_SCR.m)
 *       for each segment `points` (1:82, 83:324, 325:1031 with SCRs = SCR + [10 0 0], :23):
 *           P_s = mean(Echo_simu(1, points).^2) + eps          row 1 only, before any scaling
 *           for every row i:  P_echo = mean(echo(i, points).^2)
 *                             g = P_echo * 10^(SCRs/10) / P_s
 *                             Echo_simu(i, points) = Echo_simu(i, points) * sqrt(g)
 *       columns in no segment keep their value;
 *   echo = fun_add_clutter(Echo_simu_STC, echoData_Frame_0)                (fun_add_clutter.m)
 *       out(i, :) = Echo_simu(i, :) + echo(i, 1:point_prt): the echo may be wider than Echo_simu
 *       (clutter_ld).
 * The sums are accumulated in fp64 from the fp32 samples, eps (2^-52) is added in fp64, the gain is
 * rounded to fp32 once, the scaling product and the clutter add are fp32.  Fixed reduction order,
 * no atomics: the output is bit-identical from run to run.
 *
 * Quirks of the reference:
 *   - `.^2` of complex I/Q data is the complex square, not |x|^2, so P_s, P_echo and g are complex
 *     and sqrt(g) is the principal complex root (a result with a zero imaginary part is stored as
 *     real by MATLAB, so the root of a negative real g is +j sqrt|g|).  The function's header says
 *     it sets the SCR, so this is an oversight; both behaviours are offered:
 *       RSP_SCR_ABS2        powers are mean(|x|^2), g is real: the achieved SCR is the set one
 *                           (the native default);
 *       RSP_SCR_AS_WRITTEN  complex squares and principal root, exactly as MATLAB evaluates the
 *                           file (the default of the fun_SCR mirror in rsp/inject.py).
 *   - the body of fun_SimulateTarget(Velocity, Range, prtNum, pulse1, pulse2, pulse3) is not in
 *     the reference; only its call survives, commented out, at main.m:188.  It is defined here as
 *     a point target per segment (the model of rsp/synth.py): the segment's waveform placed at a
 *     delay column, truncated at the segment's end, and multiplied at pulse m (0-based) by
 *     exp(j dphi m), dphi = 2 pi (2 v / lambda) PRT.  Its amplitude is irrelevant (the scaling
 *     normalises it) and its modulus is constant over pulses, so row 1's power is every row's.
 *
 * rsp_scr_dev is the general form on arbitrary arrays (16 B read + 8 B written per sample).
 * rsp_inject_dev is the point-target form: Echo_simu is never materialised (8 B + 8 B per sample);
 * P_s is computed once per (CPI, segment) from the waveform and the delay.
 *   d_wf     complex64, the segments' waveforms concatenated: segment s is d_wf[wf_off[s] .. wf_off[s+1])
 *   d_delay  int32 [batch][RSP_MAX_SEG]: the waveform's first column relative to the segment's
 *            start; negative (-1) or >= seg_len: no target in that segment
 *   d_dphi   double [batch]
 * d_scr_db: double [batch], the SCR of each CPI in dB.
 * Both are asynchronous on `stream` and work on any context, the CFAR-only kind included.
 * d_out == d_simu is allowed; d_out == d_clutter only with clutter_batch == batch and clutter_ld == R;
 * any other overlap of d_out with an input is RSP_ERR_ARG, as are overlapping or out-of-range
 * segments, nseg outside 0..RSP_MAX_SEG (0: the plain add), clutter_batch outside 1..batch and NULLs.  Uses 16-byte
 * accesses when R and clutter_ld are even and the buffers 16-byte aligned, 8-byte ones otherwise
 * (the legacy R = 1031).  R <= 2^24. */
enum { RSP_SCR_ABS2 = 0, RSP_SCR_AS_WRITTEN = 1 };
typedef struct {
    int32_t nseg;                 /* <= RSP_MAX_SEG; 0: no column is scaled (fun_add_clutter alone) */
    int32_t power;                /* RSP_SCR_* */
    int32_t add_clutter;          /* 1: out = scaled target + clutter (fun_add_clutter);
                                     0: the scaled target alone (fun_SCR's return value) */
    int32_t reserved;             /* 0 */
    int64_t seg_start[RSP_MAX_SEG], seg_len[RSP_MAX_SEG];   /* disjoint, inside [0, R) */
    double  seg_db[RSP_MAX_SEG];  /* added to the SCR per segment (reference: 10, 0, 0) */
    int64_t clutter_ld;           /* clutter row pitch in elements, 0 = R (fun_add_clutter's 1:point_prt) */
    int64_t clutter_batch;        /* K clutter CPIs, CPI b uses clutter b % K; 0 = batch */
} rsp_scr_params;

int rsp_scr_dev(rsp_ctx* ctx, const void* d_simu, const void* d_clutter, void* d_out, int64_t P, int64_t R,
                int64_t batch, const double* d_scr_db /* device [batch] */, const rsp_scr_params* sp,
                void* stream);
int rsp_inject_dev(rsp_ctx* ctx, const void* d_clutter, void* d_out, int64_t P, int64_t R, int64_t batch,
                   const void* d_wf, const int64_t* wf_off /* host [nseg+1] */,
                   const int32_t* d_delay /* [batch][RSP_MAX_SEG] */, const double* d_dphi,
                   const double* d_scr_db, const rsp_scr_params* sp, void* stream);
/* Host only (no GPU, no context): the sums of x^2 (RSP_SCR_AS_WRITTEN: {re, im}) or |x|^2
 * (RSP_SCR_ABS2: {sum, ignored}) of row 1 of the target and of a clutter row over a segment of n
 * columns -> the complex gain sqrt(g) = {re, im}.  The same inline function the kernel calls. */
int rsp_scr_gain(int32_t power, const double sum_simu[2], const double sum_clutter[2], int64_t n,
                 double scr_db, double gain[2]);

/* ---- diagnostics ---------------------------------------------------------------------- */
/* Per-kernel device time accumulated from HIP events recorded on the launch stream around
 * kernel launches while profiling is enabled: enable = 1 brackets every launch, enable = N > 1
 * every N-th launch (sampling: each event pair costs the stream a few microseconds),
 * 0 stops.  Any call resets the counters.
 * Kernel ids: RSP_K_PC, RSP_K_MTD, RSP_K_CFAR_R, RSP_K_CFAR_V, and (an addition within ABI 5)
 * RSP_K_OS_V, RSP_K_OS_R for rsp_os_cfar_dev's Doppler and range launches. */
#define RSP_NKERNELS 6
enum { RSP_K_PC = 0, RSP_K_MTD = 1, RSP_K_CFAR_R = 2, RSP_K_CFAR_V = 3, RSP_K_OS_V = 4, RSP_K_OS_R = 5 };
int rsp_profile(rsp_ctx* ctx, int32_t enable);
/* Waits for the recorded events; ms[k] = summed device time, launches[k] = launch count, for
 * k < n (n <= RSP_NKERNELS entries are written; pass the length of both arrays). */
int rsp_profile_read_n(rsp_ctx* ctx, double* ms, int64_t* launches, int32_t n);
/* ABI-3 form: writes exactly 4 entries (RSP_K_PC .. RSP_K_CFAR_V), whatever RSP_NKERNELS is. */
int rsp_profile_read(rsp_ctx* ctx, double* ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* RSP_H */
