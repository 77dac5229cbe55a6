// rsp_internal.h -- argument blocks and launchers shared by the C-ABI host code (rsp_capi.cpp,
// rsp_stages.cpp, rsp_host.cpp) and the HIP kernels (one rsp_<stage>.hip per stage).  Not part
// of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <mutex>

#include "../../include/rsp.h"
#include "rsp_measure_math.h"

namespace rsp {

constexpr int kBlock = 256;  // threads per workgroup for every kernel (4 waves of 64)

// One-time launch setup of a kernel (hipFuncSetAttribute, occupancy -> resident grid), per
// device: both apply to the calling thread's current device, and contexts on different host
// threads and devices launch concurrently (rsp.h threading model), so the setup runs once per
// (kernel, device) under std::call_once and its result is cached per device.
constexpr int kMaxDevices = 64;
struct LaunchOnce {
    std::once_flag once[kMaxDevices];
    hipError_t err[kMaxDevices] = {};
    int value[kMaxDevices] = {};
};
// init(dev, &value) -> hipError_t; *value receives the cached value (e.g. resident workgroups)
template <typename F>
inline hipError_t launch_once(LaunchOnce& L, int* value, F&& init) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
    std::call_once(L.once[dev], [&] { L.err[dev] = init(dev, &L.value[dev]); });
    if (value) *value = L.value[dev];
    return L.err[dev];
}
// Dynamic-LDS attribute of a kernel (once per device).
inline hipError_t lds_attr(LaunchOnce& once, const void* kernel, size_t lds) {
    return launch_once(once, nullptr, [&](int, int*) {
        return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
}

// One pulse-compression segment as the kernel sees it (see rsp_pc_segment).
struct SegDev {
    int kind;        // RSP_SEG_FIR / RSP_SEG_MF
    int fir_shift;
    int in_start, in_len;
    int out_start, out_len;
    int nfft;
    int ntaps;
    float scale;
    const float2* H;   // MF: conj(FFT_nfft(scale*replica)) / nfft
    const float2* tw;  // MF: W_nfft^e table, e < nfft
    const float* taps_dev;  // FIR taps in device memory (no dynamic kernarg indexing)
    int ntaps4;             // ntaps rounded up to a multiple of 4
    const float2* taps2_dev;  // (scale*b_k, scale*b_k), zero-padded to ntaps4: one packed fma per tap
    float taps[RSP_MAX_FIR_TAPS];
};

struct PcArgs {
    int P, R, R_out;
    int nseg;
    int nzero;                          // output column ranges no segment writes
    int zero_lo[RSP_MAX_SEG + 1];
    int zero_hi[RSP_MAX_SEG + 1];
    SegDev seg[RSP_MAX_SEG];
};

// One matched-filter segment for every row, specialised on its FFT length; the first
// launch of a chunk also runs the FIR segment and zero-fills uncovered columns.
struct PcMfArgs {
    int R, R_out;
    int rows;
    int do_fir;
    SegDev fir;
    SegDev mf;
    // overlap-save split of a long matched filter (nsub > 1): sub-block j of a row correlates
    // input [in_start + j*sub_step, + mf.nfft) with the replica (mf.H, mf.nfft points) and keeps
    // outputs [j*sub_step, (j+1)*sub_step) -- sub_step = mf.nfft - replica length + 1, so no
    // output wraps.  nsub <= 1: the whole segment in one mf.nfft-point transform.
    int nsub, sub_step;
    // Slices of G = nfft/16 points at the end of the transform that lie past in_len (zin: known
    // zero input) / past out_len (zout: never stored) in every sub-block; 0 when the row is not
    // wave-uniform or rsp_set_pc_prune is off.  The launcher picks a pruned kernel instance from them.
    int zin, zout;
    const float* gain;   // fused iSTC (rsp_set_prefilter): echo column n scaled by gain[n], or null
    int nzero;
    int zero_lo[RSP_MAX_SEG + 1];
    int zero_hi[RSP_MAX_SEG + 1];
};

// Doppler-dimension CFAR on one column tile (Function_CFAR1D_sub on used.').
struct CfarVArgs {
    int enabled;
    int lo, hi;          // used rows [lo, hi) = rows M0+2 .. V-M0 (1-based)
    int ref, save, method;
    float T;
    float Tr;            // T / ref (threshold = max|min(window sums) * Tr)
    int cz_lo, cz_hi;    // rows zeroed before CFAR (main_cfar.m:90-91), empty if lo >= hi
    int nseg;            // column segments (fun_CFARflag); columns outside get flag 0
    int seg_lo[RSP_MAX_SEG], seg_hi[RSP_MAX_SEG];
};

// Range-dimension CFAR at the Doppler hits (executeCFAR.m:35-89).
struct CfarRArgs {
    int V, R;
    int lo, hi;          // used rows
    int rflag;
    int ref, save, method;
    float T;
    float Tr;            // T / ref
    int cz_lo, cz_hi;    // rows zeroed before CFAR
    int nseg;
    int seg_lo[RSP_MAX_SEG], seg_hi[RSP_MAX_SEG];
};

constexpr int RSP_MAX_WIN = 16;

struct MtdArgs {
    int P, R_out;
    // Sliding-window mode (main_produce_dataset_win_xzr_v2.m:117-131): launch CPI j is window
    // j % nwin of frame j / nwin; its P pulses are PC rows [n*P + win_start[j % nwin], +P) of
    // a frame-contiguous PC buffer.  nwin == 0: CPI j reads rows [j*P, (j+1)*P).
    int nwin;
    int win_start[RSP_MAX_WIN];
    int pin;             // pulses per CPI and beam (<= P; the FFT zero-pads rows pin..P-1)
    int mti_lag;         // fused MTI (rsp_set_prefilter): pulse p reads row p+lag minus row p, 0 past pin-lag
    int beams;           // 2: DMX pair -- RDM = |X_0| + |X_1|, diff (if non-null) = |X_1| - |X_0|
    float* diff;
    // Bluestein plan for P without a radix plan (v2 native P = 332): bnf > 0 is the power-of-
    // two convolution length, bwc[n] = w[n] exp(-j pi n^2/P) (0 for n >= P), bspec = FFT of the
    // conjugate chirp / bnf; tw is then the bnf-point twiddle table.
    int bnf;
    const float2* bwc;
    const float2* bspec;
    int shift;           // fftshift offset floor(P/2), or 0
    int z_lo, z_hi;      // fun_0v_pressing rows zeroed in the RDM
    const float* win;    // slow-time window, P entries
    const float2* tw;    // W_P^e table
    CfarVArgs cv;
    // Fused range-CFAR front end (cv.enabled): the MTD kernel writes the final flag plane's
    // background -- flagV itself when rflag == 0, zeros otherwise -- and appends every
    // in-band Doppler hit (linear cell index within the launch) to `hits`; cfar_hits_kernel
    // then sets the re-localised range detections.  flagV is written only when requested.
    uint8_t* flag;
    int rflag;
    int flag_zero;         // rflag: the MTD kernel writes the flag plane's zeros (else the host memsets it)
    uint32_t* hits;        // workgroup b owns hits[b*W*P, (b+1)*W*P) (its own cells: no overflow)
    uint32_t* hit_count;   // hit_count[b] = entries of workgroup b (b = blockIdx.y*gridDim.x + blockIdx.x)
    uint32_t cell_off;     // added to every hit index (grouped range stages: the chunk's offset in its group)
    // The previous chunk's range stage, run by extra workgroups of this launch (same stream,
    // so that chunk's RDM and hit lists are complete): prev_nregions == 0 means none.
    const float* prev_rdm;
    uint8_t* prev_flag;
    const uint32_t* prev_hits;
    const uint32_t* prev_count;
    int prev_nregions, prev_region;
    CfarRArgs prev_cr;
};


// Raw-data ingest (rsp_ingest.hip): one frame of uniform DDC PRT records.
// MeasureArgs (motionParaMeasure.m's scalar arguments): rsp_measure_math.h.
// Workgroups per CPI for the hit lists (1: hits_kernel; > 1: the banded path, which needs
// batch * nb * R int32 of scratch in band_cnt).
int measure_bands(int V, int batch);
hipError_t launch_measure(const float* sum, const float* diff, const uint8_t* flag, int V, int R, int batch,
                          const MeasureArgs& a, const double* r_scale, const double* v_scale, int64_t max_hits,
                          double* est, int32_t* cells, int32_t* count, int32_t* band_cnt, int nb, hipStream_t st);

// The hit list alone (hits_kernel): list[(cpi * max_hits + i) * 3] = cell v*R + c of hit i in find()
// order (the other two words of a slot are not written), count[cpi * 2] = the CPI's hits.
hipError_t launch_hit_list(const uint8_t* flag, int V, int R, int batch, int64_t ld, int64_t cs, int64_t max_hits,
                           int64_t* list, int32_t* count, hipStream_t st);

// Plot condensation (rsp_condense.hip): rsp_condense_params with the shape and the resolved pitches.
struct CondenseArgs {
    int V, R;
    int gap_v, gap_r, wrap_v;
    int max_plots;    // records per CPI in d_plots
    int list_cap;     // (launch_condense) slots per CPI of the peaks' hit list
    int tw;           // (launch_condense) 16-column segments per row of a dense tile
    int64_t ld, cs;   // row pitch and CPI stride of the amplitude / flag / peak planes, in elements
    size_t cells;     // V * R
};
// Scratch bytes per CPI of a launch_condense chunk (a multiple of 16).
size_t condense_scratch_per_cpi(int64_t V, int64_t R, int32_t max_plots);
// One chunk of CPIs (at most 65535); plots may be null; scratch holds batch * condense_scratch_per_cpi bytes.
hipError_t launch_condense(const float* amp, const uint8_t* flag, uint8_t* peak, int batch, CondenseArgs a,
                           int32_t* plots, int32_t* count, void* scratch, hipStream_t st);

// Clutter map (rsp_cmap.hip): rsp_cmap_params with the shape, the resolved pitches and the plan.
struct CmapArgs {
    int P, R, K, kpad;
    int beams;
    int kb, vec, split;   // the band kernel instance (rsp_cmap_plan_t)
    int warmup, hold, slots;
    float T, w;
    int64_t ld, cs;       // row pitch and CPI stride of the PC rows, in complex elements
};
// The instance a shape takes; vec from the shape alone (launch_cmap_band also looks at the pointers).
void cmap_plan(int64_t P, int64_t R, int64_t K, int64_t ld, int64_t cs, int* kb, int* passes, int* vec, int* split);
// band[b][k][r] for b < batch (at most 65535); tab: float2 [P][kpad].
hipError_t launch_cmap_band(const float2* pc, const float2* tab, const CmapArgs& a, int batch, float* band,
                            hipStream_t st);
// The recursion over the batch's CPIs in order, then the ages.
hipError_t launch_cmap_update(const float* band, const int32_t* slot, const CmapArgs& a, int64_t batch, float* map,
                              int32_t* age, uint8_t* flag, hipStream_t st);

// Doppler line width (rsp_width.hip): rsp_width_params with the shape and the resolved pitches.
struct WidthArgs {
    int V, R;
    int interp, shift;
    int lg, pitch;    // (launch_width) log2 of a lane's chunk of rows; padded LDS elements per column
    double level;     // 10^(amp_constr / 20)
    int64_t ld, cs;   // row pitch and CPI stride of the amplitude / flag planes, in elements
};
// A lane's chunk of rows (1 << *lg, 64 chunks cover V) and the chunk-padded LDS elements of a column.
void width_geometry(int V, int* lg, int* pitch);
// Dynamic LDS of a width_kernel workgroup: four columns of V floats and, with interp > 1, V doubles,
// chunk-padded.
size_t width_lds_bytes(int V, int interp);
// span [batch][R][2], count [batch] (batch at most 65535); flag may be null (every column).
hipError_t launch_width(const float* amp, const uint8_t* flag, int batch, const WidthArgs& a, int32_t* span,
                        int32_t* count, hipStream_t st);

// Ordered-statistic CFAR (rsp_oscfar.hip): one 1-D test (rank k of a window of ref cells beyond save
// guard cells, threshold T) per stage, and the planes' geometry.
enum { kOsGo = 0, kOsSo = 1, kOsUnion = 2 };
struct OsTest {
    int ref, save, k, form;   // form: kOsGo / kOsSo (per side), kOsUnion (both sides as one set)
    float T;
};
struct OsArgs {
    int V, R;
    int lo, hi;            // band rows
    int cz_lo, cz_hi;      // rows read as zero
    int nseg;
    int seg_lo[RSP_MAX_SEG], seg_hi[RSP_MAX_SEG];
    int rflag;
    OsTest v, r;
    int64_t ld, cs;        // row pitch and CPI stride of the RDM and flag planes, in elements
    int64_t fv_ld, fv_cs;  // those of the flagV plane (the caller's window, or the dense scratch)
};
constexpr int kOsRTile = 1024;   // columns per range workgroup
// The Doppler tile of a V-row plane: log2 of its columns and the LDS floats between them.
void os_v_geometry(int V, int* lw, int* pitch);
size_t os_v_lds_bytes(int V);
// Dynamic LDS of a range workgroup: the tile and a halo of save + ref + 2 columns on each side,
// 10 bytes per column.
size_t os_r_lds_bytes(const OsTest& r);
// flagV (and, with a.rflag == 0, flag; either may be null) of batch CPIs (at most 65535).
hipError_t launch_os_v(const float* rdm, uint8_t* flag, uint8_t* flagV, int batch, const OsArgs& a, hipStream_t st);
// flag from flagV (a.rflag == 1).
hipError_t launch_os_r(const float* rdm, const uint8_t* flagV, uint8_t* flag, int batch, const OsArgs& a,
                       hipStream_t st);

// Tracking (rsp_track.hip): rsp_track_params with the shape and the gate weights.
struct TrackArgs {
    int T, H;              // max_tracks, max_hits
    int M, N, drop_t, drop_c;
    int slots;
    int lanes;             // (launch_track) lanes that share a track's scan of the plots: track_lanes(T)
    double dt, rate_sign, gate_r, gate_v;
    double wr, wv;         // 1 / gate^2, fp64 on the host
    double alpha_r, alpha_v, alpha_e;
};
// Dynamic LDS of a track_kernel workgroup, 56 B per entry and 32 B per plot, and the most it may ask for.
size_t track_lds_bytes(int64_t T, int64_t H);
size_t track_lds_max();
// A power of two, 1..64: 1024 threads over the entries rounded up to a power of two.
int track_lanes(int T);
// One workgroup per slot walks the batch; slot, dt, snap_f / snap_i may be null.
hipError_t launch_track(const double* est, const int32_t* count, int64_t batch, const TrackArgs& a, const int32_t* slot,
                        const double* dt, double* state_f, int32_t* state_i, int32_t* meta, int32_t* assign,
                        double* snap_f, int32_t* snap_i, int32_t* tcount, hipStream_t st);

// Post-detection integration (rsp_integ.hip): rsp_integ_params with the shape and the resolved pitches.
struct IntegArgs {
    int V, R;
    int n, m, spread;      // m, spread: the binary form's (0 for the sum)
    int slots;
    int64_t ld, cs;        // row pitch and CPI stride of the input and output planes, in elements
};
// The plan table of a call: batch rows of n + 3 ints.
size_t integ_plan_bytes(int64_t batch, int n);
// Plan, integrate, ring update.  shift, slot, neff may be null; hist only when n == 1.
hipError_t launch_integ_sum(const float* in, float* hist, const int32_t* shift, const int32_t* slot, int32_t* meta,
                            int32_t* plan, float* out, int32_t* neff, int64_t batch, const IntegArgs& a, hipStream_t st);
hipError_t launch_integ_bin(const uint8_t* in, uint8_t* hist, const int32_t* shift, const int32_t* slot, int32_t* meta,
                            int32_t* plan, uint8_t* out, int32_t* neff, int64_t batch, const IntegArgs& a, hipStream_t st);

// Stacked-beam fusion (rsp_fuse.hip): rsp_fuse_params with the shape and the resolved strides.
struct FuseArgs {
    int V, R;
    int beams, min_beams, law;
    int64_t ld, bs, cs;    // row pitch, beam stride and CPI stride of the input planes, in elements
    double beam_el[32];
};
// One streaming launch per 2^30 workgroups.  famp, fcnt may be null.
hipError_t launch_beam_fuse(const float* amp, const uint8_t* flag, uint8_t* fflag, uint8_t* fbeam, float* famp,
                            uint8_t* fcnt, int64_t batch, const FuseArgs& a, hipStream_t st);
// One thread per slot of the hit lists; blocks of 256 slots per CPI.  hb may be null.
int64_t beam_elev_blocks(int64_t batch, int64_t max_hits);
hipError_t launch_beam_elev(const float* amp, const uint8_t* flag, const uint8_t* fbeam, const int32_t* cells,
                            const int32_t* count, int64_t max_hits, double* el, int64_t el_stride, int32_t* hb,
                            int64_t batch, const FuseArgs& a, hipStream_t st);

// Detection scoring (rsp_score.hip): rsp_score_params with the shape and the resolved pitches.
struct ScoreArgs {
    int V, R;
    int hv, hr, n_cell, v_lim, r_lim;
    int64_t ld, cs;   // row pitch and CPI stride of the flag / RDM planes, in elements
};
// rec [batch][8] int32 (rsp.h); rdm may be null (no peak search).
hipError_t launch_score(const uint8_t* flag, const float* rdm, const int32_t* truth, int32_t* rec, int batch,
                        const ScoreArgs& a, hipStream_t st);

// Echo pre-filters (rsp_prefilter.hip): iSTC gain per range bin and/or MTI row difference.
hipError_t launch_prefilter(const float2* in, float2* out, const float* gain, int P, int R, int64_t batch, int lag,
                            hipStream_t st);

// Target injection at a set SCR (rsp_inject.hip): fun_SCR.m / fun_add_clutter.m.
// 10^(SCR/10), the power ratio of a SCR in dB (fun_SCR.m:23).
__host__ __device__ inline double scr_lin(double scr_db) { return pow(10.0, scr_db / 10.0); }
// The gain sqrt(g) of one (row, segment) from the sums of x^2 (RSP_SCR_AS_WRITTEN: complex) or
// |x|^2 (RSP_SCR_ABS2: real, the imaginary sums are ignored) over the segment's n columns and
// the ratio k = scr_lin(SCR):
//   P_s = mean(simu row 1) + eps, P_echo = mean(clutter row), g = P_echo * k / P_s,
// and the principal root.  MATLAB stores a result whose imaginary part is zero as real, so the
// root of a negative real g is +j sqrt|g| whatever the sign of that zero.  The row kernel and the
// host export rsp_scr_gain both call this (and scr_lin).
__host__ __device__ inline void scr_gain(int power, double ss_re, double ss_im, double sc_re, double sc_im, double n,
                                         double k, double* g_re, double* g_im) {
    const double eps = 2.220446049250313e-16;   // MATLAB's eps, 2^-52
    const double ps_re = ss_re / n + eps, pe_re = sc_re / n * k;
    double q_re, q_im = 0.0;
    if (power == RSP_SCR_AS_WRITTEN) {
        const double ps_im = ss_im / n, pe_im = sc_im / n * k;
        const double den = ps_re * ps_re + ps_im * ps_im;
        q_re = (pe_re * ps_re + pe_im * ps_im) / den;
        q_im = (pe_im * ps_re - pe_re * ps_im) / den;
    } else {
        q_re = pe_re / ps_re;
    }
    const double r = sqrt(q_re * q_re + q_im * q_im);   // |g| stays far inside the fp64 range
    if (r == 0.0) {
        *g_re = 0.0;
        *g_im = 0.0;
    } else if (q_re >= 0.0) {
        const double t = sqrt(0.5 * (r + q_re));
        *g_re = t;
        *g_im = q_im / (2.0 * t);
    } else {
        const double t = sqrt(0.5 * (r - q_re));
        *g_re = fabs(q_im) / (2.0 * t);
        *g_im = q_im < 0.0 ? -t : t;
    }
}

struct InjectArgs {
    int P, R;
    int nseg, power, add;
    int lo[RSP_MAX_SEG], hi[RSP_MAX_SEG];   // segment columns [lo, hi)
    double db[RSP_MAX_SEG];
    int64_t c_ld, c_cs;                     // clutter row pitch and CPI stride, in elements
    int c_batch;                            // CPI b reads clutter CPI b % c_batch
    const float2* simu;                     // general form; null in the point-target form
    const float2* clutter;
    float2* out;
    const double* scr_db;                   // [batch]
    // context scratch, inject_ps_stride(P) doubles per CPI: [RSP_MAX_SEG][4] = {row 1's sums re, im,
    // scr_lin(SCR + seg_db), 0}, then (point-target form) [P][2] = cos, sin of dphi * m
    double* ps;
    // point-target form
    const float2* wf;
    int wf_off[RSP_MAX_SEG + 1];
    const int32_t* delay;                   // [batch][RSP_MAX_SEG]
    const double* dphi;                     // [batch]
};
// Complex samples of a row the row kernel keeps in registers per thread; longer rows are read a
// second time (from L2) for the scaling pass.
constexpr int kInjectRegVec = 8;            // 8- or 16-byte accesses per thread
constexpr int64_t inject_ps_stride(int64_t P) { return 4 * RSP_MAX_SEG + 2 * P; }
// vec16: 16-byte accesses (R, c_ld even and the buffers 16-byte aligned)
hipError_t launch_inject(const InjectArgs& a, int64_t batch, bool vec16, hipStream_t st);

struct IngestArgs {
    int prt_num, point_prt, channel_num, beam_num;
    int bytes_head, bytes_realtime, bytes_tail;
    int64_t rec_bytes;       // head + realtime + payload (padded to 64 B) + tail of a DDC record
    int64_t beam_stride;     // output elements between consecutive beams' [prt][sample] planes
    int ddc_only;            // rsp_ingest_ddc_dev: records sized by the params, other types refused
    int64_t* offs;           // [prt_num] record offsets in the stream (check -> decode kernel)
    int32_t* types;          // [prt_num] data types of the decoded records
    int dbf_lds;             // (launch_ingest) generic-shape decode: the DBF matrix staged in LDS
};
hipError_t launch_ingest(const uint8_t* stream, int64_t nbytes, const IngestArgs& a, const float2* dbf,
                         float2* out, uint16_t* servo, int32_t* status, hipStream_t s);

// Legacy two-beam 24-bit records (rsp_ingest_legacy.hip): frameDataRead_A_xzr.m / Show_Read.m.
constexpr int kLegacyHeadBytes = 28, kLegacyGroupBytes = 12, kLegacyTailBytes = 8;
constexpr int64_t legacy_record_bytes(int64_t point_prt) {
    return kLegacyHeadBytes + kLegacyGroupBytes * point_prt + kLegacyTailBytes;
}
// Rows (frame x PRT, in stream order) whose head and payload lie inside nbytes: the reference
// stores a row before it skips the tail, so a row with only its tail cut still counts.
constexpr int64_t legacy_rows_decoded(int64_t nbytes, int64_t rec_bytes, int64_t rows) {
    const int64_t n = (nbytes + kLegacyTailBytes) / rec_bytes;   // (r + 1) * rec - tail <= nbytes
    return n < rows ? n : rows;
}
struct LegacyIngestArgs {
    int prt_num, point_prt, nframes;
    int64_t rows;                       // nframes * prt_num
    int64_t rows_decoded;               // legacy_rows_decoded: rows from here on are zeros
    int64_t rec_bytes, nbytes;
    int64_t beam_stride, frame_stride;  // output elements between the two beams' planes / between frames
};
// status: int32 [rows + 1]; angle ([rows]) and head ([rows][RSP_LEGACY_HEAD_FIELDS]) may be null.
hipError_t launch_ingest_legacy(const uint8_t* stream, const LegacyIngestArgs& a, float2* out, double* angle,
                                int32_t* head, int32_t* status, hipStream_t s);

// Payload bytes of one record by data type (FrameDataRead_xzr.m:104-119): ADC (0) int16 per
// channel, DDC (1) int16 I/Q per channel, anything else the 24-bit DBF layout (3-byte I/Q per
// channel plus 8 - mod(6*ch, 8) pad bytes per sample), the whole padded to 64 B.
constexpr int64_t ingest_payload_bytes(uint32_t type, int64_t pdn, int64_t ch) {
    const int64_t sig = type == 0 ? pdn * ch * 2
                      : type == 1 ? pdn * ch * 4
                                  : pdn * ch * 6 + pdn * (8 - (6 * ch) % 8);
    return sig % 64 ? sig + 64 - sig % 64 : sig;
}
// 24-bit DBF branch (FrameDataRead_xzr.m:130-135,162-164): bytes per sample row, and the number
// of values the three column ranges 1:3:end-3, 2:3:end-2, 3:3:end give (-1 when their lengths
// differ or the count is odd: the reference's own sum or I/Q pairing raises a size error).
constexpr int dbf24_row_bytes(int ch) { return 6 * ch + (8 - (6 * ch) % 8); }
constexpr int dbf24_values(int ch) {
    const int L = dbf24_row_bytes(ch);
    const int n1 = L - 3 >= 1 ? (L - 4) / 3 + 1 : 0, n2 = L - 2 >= 2 ? (L - 4) / 3 + 1 : 0, n3 = L / 3;
    return (n1 == n2 && n2 == n3 && n1 % 2 == 0) ? n1 : -1;
}

bool mtd_size_supported(int P, int beams = 1);
bool pc_nfft_supported(int n);
size_t pc_lds_bytes(int max_nfft);

hipError_t launch_pc(const void* echo, int dtype, float2* out, int64_t rows, const PcArgs& a,
                     size_t lds_bytes, hipStream_t s);
// float2 slots the FIR stages in the row's LDS slot: ntaps4-1 leading zeros, the segment,
// and the 4-output block's read-ahead
inline int fir_stage_len(const SegDev& g) { return g.ntaps4 - 1 + g.out_len + 4; }
bool pc_mf_supported(int nfft, int fir_stage_len);
bool pc_pair_supported(int nfft1, int nfft2);
// The pruned kernel instance launch_pc_mf runs for (a1, a2), as 0x<ZIN1><ZOUT1><ZIN2><ZOUT2>
// (pc_row); 0: the generic instance
int pc_prune_select(const PcMfArgs& a1, const PcMfArgs* a2);
// Consecutive units a long-row workgroup slot of launch_pc_mf(a1, a2) walks when `want` (1, 2, 4)
// are asked for: `want` where the multi-row path exists (4096-point rows without a FIR), else 1
int pc_rows_select(const PcMfArgs& a1, const PcMfArgs* a2, int want);
// a2 == nullptr: one segment; otherwise both segments (a1.mf.nfft, a2->mf.nfft) in one launch;
// pc_rows: rows per long-row workgroup slot asked for (pc_rows_select decides)
hipError_t launch_pc_mf(const void* echo, int dtype, float2* out, const PcMfArgs& a1, const PcMfArgs* a2,
                        int pc_rows, hipStream_t s);
hipError_t launch_mtd(const float2* pc, float* rdm, uint8_t* flagV, int ncpi, const MtdArgs& a,
                      hipStream_t s);
// Doppler CFAR straight from an RDM ([ncpi][V][R] fp32) for rsp_cfar.
hipError_t launch_cfar_v(const float* rdm, uint8_t* flagV, int ncpi, int V, int R,
                         const CfarVArgs& a, hipStream_t s);
// Range CFAR + re-localisation at the Doppler hits listed by the MTD kernel (scatter form of
// executeCFAR.m:45-84).  `zero_slot` (if non-null) is reset for a later launch.
hipError_t launch_cfar_hits(const float* rdm, uint8_t* flag, const uint32_t* hits, const uint32_t* counts,
                            int nregions, int region, const CfarRArgs& a, hipStream_t s);
// The choices the launchers make, as pure host functions that rsp_cfar_plan reports too:
// the hit kernel of launch_cfar_hits (RSP_HITS_*; *lpr its lanes per region, 0 for the per-hit kernels)
int cfar_hits_select(const CfarRArgs& a, int nregions, int region, int* lpr);
// the range kernel of launch_cfar_r (RSP_CFAR_R_*; *groups its workgroups per row, 0 where one covers a row)
int cfar_r_select(const CfarRArgs& a, int* groups);
// log2 of cfar_v_kernel's tile width
int cfar_v_tile_log2(int V);
// launch_mtd: the compiled 5 + 7 Doppler window (else the runtime-window instance), and whether the
// previous chunk's range stage (a.prev_*) rides as RangeJob57 (else as prev_chunk_hits)
bool mtd_window_compiled(const MtdArgs& a);
bool mtd_range_job57(const MtdArgs& a);
// range bins and threads of one MTD workgroup (false: no instance for P / beams)
bool mtd_geometry(int P, int beams, int* W, int* T);
// MTD workgroups per launch and cells per workgroup (hit-list regions)
void mtd_regions(int P, int R_out, int ncpi, int* nregions, int* region, int beams = 1);
// Bluestein convolution length for a P without a radix plan (0: unsupported)
int mtd_bluestein_nf(int P);
hipError_t launch_cfar_r(const float* rdm, const uint8_t* flagV, uint8_t* flag, int ncpi,
                         const CfarRArgs& a, hipStream_t s);
// Whether launch_cfar_r has a kernel for the row length / window (the generic kernel stages a
// row in LDS: 10 bytes per cell)
bool cfar_r_supported(const CfarRArgs& a);
// dtype/layout conversion of a host-API input into [batch][P][R] complex float32.
hipError_t launch_canon(const void* in, int dtype, int layout, float2* out, int64_t batch,
                        int P, int R, hipStream_t s);
// [batch][A][B] -> [batch][B][A] for 4-byte and 1-byte elements.
hipError_t launch_transpose_f32(const float* in, float* out, int64_t batch, int A, int B,
                                hipStream_t s);
hipError_t launch_transpose_u8(const uint8_t* in, uint8_t* out, int64_t batch, int A, int B,
                               hipStream_t s);
// One plane's sub-block transpose: element (a, b), a < A, b < B, of in[a*in_pitch + b] to
// out[b*out_pitch + a] (elements: RSP_SUB_*; C32F16 widens to complex float).  The host path's
// pieces: either pointer may be pinned host memory.
enum { RSP_SUB_F32 = 0, RSP_SUB_U8 = 1, RSP_SUB_C64 = 2, RSP_SUB_C32F16 = 3 };
hipError_t launch_transpose_sub(int elem, const void* in, void* out, int A, int B, size_t in_pitch, size_t out_pitch,
                                hipStream_t s);
// nwords 4-byte words in -> out (either may be pinned host memory)
hipError_t launch_copy_words(const void* in, void* out, size_t nwords, hipStream_t s);

}  // namespace rsp
