// rsp_mtd.hip -- moving-target detection, the second kernel of the range-Doppler chain (gfx950).
//
//   mtd_kernel     one workgroup per tile of W range bins x all P pulses: slow-time window,
//                  P-point FFT per range bin, fftshift, |.|, fun_0v_pressing, then the
//                  Doppler-dimension CA-CFAR on the same columns while they sit in LDS
//                  (MTD/fun_Process_MTD.m:13-40, MTD/fun_0v_pressing.m:13-24,
//                   CFAR_WangCai/executeCFAR.m:23-31 with Function_CFAR1D_sub.m:17-69).
//   mtd_bluestein_kernel  the same for a pulse count without a radix plan.
#include <hip/hip_runtime.h>

#include "rsp_fft.h"
#include "rsp_buf.h"
#include "rsp_diag.h"
#include "rsp_internal.h"
#include "rsp_cfar_dev.h"

namespace rsp {

// ================================================================== MTD (+ Doppler CFAR)
// One workgroup = W range bins x all P pulses.  Thread (c, g): range bin c of the tile,
// pulses g + G*m (m < E) -- the strided pattern of fft_reg, so the pulse-compressed
// samples load straight into registers with W-wide coalesced rows, the slow-time FFT
// runs register-resident with LDS exchanges, and |X| leaves in coalesced RDM rows.
template <int P, int BEAMS = 1>
struct MtdCfg {
    // elements per thread: 16 (24 for the 3*2^k lengths); from P = 512 on (one beam) the
    // workgroup grows with G (512..1024 threads) so a tile keeps >= 8..16 range bins
    // (>= 64..128-B row segments) and a thread still holds 16 elements -- E = 32 at 256 threads
    // needed 169 VGPRs, 2 waves per SIMD
    static constexpr int E = (P % 3 == 0) ? 24 : 16;
    static constexpr int G = P / E;                    // threads per range bin
    // threads per workgroup (512 for P = 256 measured neutral at c4: 529 vs 523 us per launch)
    static constexpr int T = (BEAMS == 1 && P >= 512 && P % 3 != 0) ? (G * 16 < 1024 ? G * 16 : 1024) : kBlock;
    // minimum waves per SIMD (__launch_bounds__' second argument): two 512-thread workgroups
    // per CU need <= 128 VGPRs
    static constexpr int WPE = T == 512 ? 4 : 1;
    static constexpr int W = T / G;                    // range bins per workgroup
    static constexpr int SLOT = padded_len(P);         // FFT exchange slot (float2)
    static constexpr int MS = P + 1;                   // odd float stride of a CFAR column
    static constexpr int SPAD = 32;                    // sums pad: save + ref + 2 <= 32 (host-checked)
    static constexpr int SMS = P + 2 * SPAD + 1;       // padded sums column (odd stride)
    static constexpr size_t lds_fft = (size_t)W * SLOT * sizeof(float2);
    static constexpr size_t lds_cfar = (size_t)W * (MS + SMS) * sizeof(float);
    static constexpr size_t lds = lds_fft > lds_cfar ? lds_fft : lds_cfar;
    // REF > 0: the window sums stay in registers; LDS holds only a padded magnitude column
    // (SPAD pad cells on each side, odd stride), inside the FFT exchange area
    static constexpr int MS2 = P + 2 * SPAD + 1;
    static constexpr size_t lds_cfar_reg = (size_t)W * MS2 * sizeof(float);
    static constexpr size_t lds_reg = lds_fft > lds_cfar_reg ? lds_fft : lds_cfar_reg;
    template <int REF>
    static constexpr size_t lds_for() { return REF > 0 ? lds_reg : lds; }
    static_assert(G * E == P && (G & (G - 1)) == 0 && G <= T, "MTD tiling");
};

// Per-row outputs of the Doppler CFAR at cell (v, r) of launch CPI `cpi`: flagV (if requested),
// the flag plane's background (flagV when the range stage is off, else 0) and, for a hit
// with the range stage on, an entry in the hit list (one atomic per wave and row).
struct DopplerOut {
    __amdgpu_buffer_rsrc_t fv, fl;   // flagV / flag planes of this CPI (num_records 0 if absent)
    uint32_t vo;                     // this lane's cell offset (row v0, column r) or kOob
    uint32_t R;
    uint32_t* hits;                  // this workgroup's region of the hit list
    uint32_t* lds_count;             // workgroup hit counter (LDS)
    uint32_t cell0;                  // linear index of (v0, r) within the launch
    bool want_fv, fused, rflag;
    bool zero_bg;                    // rflag: write the flag plane's zero background here
};

// The Doppler-stage outputs of a thread's run of N rows (bit i of `mask` = row v0+i is a hit);
// called with every lane of the wave active (its ballots and prefix-sum shuffles read all lanes):
// flagV / flag bytes where requested (uniform branches, once per run), and the hits appended to
// the workgroup's list.  Hits are sparse, so the append path is entered only by waves that
// have one: one ballot over the masks, then per row one ballot and one LDS atomic per wave.
template <int N, typename Hit>
__device__ __forceinline__ void doppler_emit(const DopplerOut& o, bool anyhit, const Hit& hit) {
    if (o.want_fv) {
#pragma unroll
        for (int i = 0; i < N; ++i) buf_st_u8(hit(i) ? 1u : 0u, o.fv, o.vo, (uint32_t)i * o.R);
    }
    if (!o.fused) return;
    if (!o.rflag) {   // flag = flagV (executeCFAR.m:91)
#pragma unroll
        for (int i = 0; i < N; ++i) buf_st_u8(hit(i) ? 1u : 0u, o.fl, o.vo, (uint32_t)i * o.R);
        return;
    }
    if (o.zero_bg) {   // zero background (here, or pre-zeroed); the range stage sets the detections
#pragma unroll
        for (int i = 0; i < N; ++i) buf_st_u8(0, o.fl, o.vo, (uint32_t)i * o.R);
    }
    if (__ballot(anyhit) == 0) return;   // the common case: no hit in the wave's rows
    // row by row: one ballot per row of the run gives the row's hit lanes, so the wave's
    // entries go out row-major -- each store instruction writes the row's hits as one
    // contiguous run (a lane-major run per lane made every store a scatter), and neighbouring
    // entries are neighbouring columns of one row, whose range windows overlap.  The
    // counts are scalar (popcounts of the ballots, each taken once): one LDS atomic per wave,
    // its result broadcast by readfirstlane (no shuffle through LDS).
    uint64_t bal[N];
    uint32_t total = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        bal[i] = __ballot(hit(i));
        total += (uint32_t)__popcll(bal[i]);
    }
    uint32_t base = 0;
    if (__lane_id() == 0) base = atomicAdd(o.lds_count, total);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint64_t b = bal[i];
        if (b == 0) continue;   // (wave-uniform)
        if (hit(i)) {
            const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            uint32_t* dst = o.hits + base + below;
            *dst = o.cell0 + (uint32_t)i * o.R;
        }
        base += (uint32_t)__popcll(b);
    }
}

// the same for a row bit mask (bit i = row v0+i is a hit)
template <int N>
__device__ __forceinline__ void doppler_emit_mask(const DopplerOut& o, uint32_t mask) {
    doppler_emit<N>(o, mask != 0u, [&](int i) { return ((mask >> i) & 1u) != 0u; });
}

template <int N>
__device__ __forceinline__ void doppler_flags(const float* mag, const float* sums, const CfarVArgs& cv, bool col_on,
                                              int v0, int v1, const DopplerOut& o) {
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (v0 + i < v1 && doppler_test(mag, sums, cv, col_on, v0 + i)) mask |= 1u << i;
    doppler_emit_mask<N>(o, mask);
}

// Doppler CFAR with the reference's window compiled in (REF = 5 reference and SAVE = 7 guard
// cells, main_cfar.m:40-58; other windows take the runtime path; the method and the row band
// stay runtime).  A thread owns a run of E rows of one range column: it reads its rows and the
// (left, right) window cells of every row as pairs from the padded magnitude column -- the two
// cells of a pair lie 2 SAVE + REF + 1 apart, one ds_read2 into a register pair -- and forms each
// row's two window sums together with packed adds (each sum still the left-to-right add of its
// REF cells, mean()'s order), in registers: no sums array, no second barrier, and the LDS
// footprint stays inside the FFT exchange area.
template <int P, int REF, int BEAMS>
__device__ __forceinline__ void doppler_cfar_fixed(const float* mag, const CfarVArgs& cv, bool col_on, int v0,
                                                   const DopplerOut& o) {
    static_assert(REF == 5, "the compiled-in window is the reference's (5 reference, 7 guard cells)");
    constexpr int SAVE = 7;
    // mag: this column's magnitudes, mag[v] for v in [-SPAD, P + SPAD) (pad cells unused:
    // every row in [lo, hi) has at least one window inside the column, the other is selected
    // away).  The left window of row v0+i starts at v0+i-SAVE-REF, the right one at
    // v0+i+SAVE+1.
    constexpr int E = MtdCfg<P, BEAMS>::E, NL = E + REF - 1, DLR = 2 * SAVE + REF + 1;
    const float* bl = mag + v0 - SAVE - REF;
    v2f lr[NL];   // (left cell, right cell) of window position i: bl[i], bl[i + DLR]
    float m[E];   // the cells under test, bl[SAVE + REF + i]: inside the pairs' span
    if constexpr (NL == 20 && DLR == 20) {
        // one asm block: 20 ds_read2_b32 straight into the pairs (hipcc merges neighbouring
        // cells instead and spends ~40 v_mov re-pairing them), and the wait on them
        const uint32_t ad = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)bl;
#define RSP_PAIR_LD(i, j) "ds_read2_b32 %" #i ", %20 offset0:" #i " offset1:" #j "\n\t"
        asm volatile(RSP_PAIR_LD(0, 20) RSP_PAIR_LD(1, 21) RSP_PAIR_LD(2, 22) RSP_PAIR_LD(3, 23) RSP_PAIR_LD(4, 24)
                     RSP_PAIR_LD(5, 25) RSP_PAIR_LD(6, 26) RSP_PAIR_LD(7, 27) RSP_PAIR_LD(8, 28) RSP_PAIR_LD(9, 29)
                     RSP_PAIR_LD(10, 30) RSP_PAIR_LD(11, 31) RSP_PAIR_LD(12, 32) RSP_PAIR_LD(13, 33)
                     RSP_PAIR_LD(14, 34) RSP_PAIR_LD(15, 35) RSP_PAIR_LD(16, 36) RSP_PAIR_LD(17, 37)
                     RSP_PAIR_LD(18, 38) RSP_PAIR_LD(19, 39) "s_waitcnt lgkmcnt(0)"
                     : "=&v"(lr[0]), "=&v"(lr[1]), "=&v"(lr[2]), "=&v"(lr[3]), "=&v"(lr[4]), "=&v"(lr[5]), "=&v"(lr[6]),
                       "=&v"(lr[7]), "=&v"(lr[8]), "=&v"(lr[9]), "=&v"(lr[10]), "=&v"(lr[11]), "=&v"(lr[12]),
                       "=&v"(lr[13]), "=&v"(lr[14]), "=&v"(lr[15]), "=&v"(lr[16]), "=&v"(lr[17]), "=&v"(lr[18]),
                       "=&v"(lr[19])
                     : "v"(ad)
                     : "memory");
#undef RSP_PAIR_LD
#pragma unroll
        for (int i = 0; i < E; ++i) m[i] = SAVE + REF + i < NL ? lr[SAVE + REF + i].x : lr[SAVE + REF + i - DLR].y;
    } else {
#pragma unroll
        for (int i = 0; i < NL; ++i) lr[i] = (v2f){bl[i], bl[i + DLR]};
#pragma unroll
        for (int i = 0; i < E; ++i) m[i] = bl[SAVE + REF + i];
    }
    const int kl = cv.lo + SAVE + REF - v0;     // row v0+i has a left window iff i >= kl
    const int kr = cv.hi - SAVE - 1 - REF - v0; // ... and a right window iff i <= kr
    const int b0 = cv.lo - v0, b1 = cv.hi - v0; // tested rows: b0 <= i < b1
    const bool go = cv.method == 0;
    // per-row hit predicates (lane masks, not a packed bit mask: each row's ballot is then the
    // compare's own result, with no bit packing and extraction around it)
    bool h[E];
    if (kl <= 0 && kr >= E - 1 && b0 <= 0 && b1 >= E && go) {
        // the common case: every row of the run is tested and has both windows (GO): the same
        // sums, the greater of the two (magnitude sums are never NaN or -0, so max is the
        // compare-select), without the per-row window and band selects
#pragma unroll
        for (int i = 0; i < E; ++i) {
            v2f sw = lr[i];
#pragma unroll
            for (int q = 1; q < REF; ++q) sw += lr[i + q];
            h[i] = col_on & (m[i] >= __builtin_fmaxf(sw.x, sw.y) * cv.Tr);
        }
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i) {
            v2f sw = lr[i];
#pragma unroll
            for (int q = 1; q < REF; ++q) sw += lr[i + q];
            const float sl = sw.x, sr = sw.y;
            const bool lok = i >= kl, rok = i <= kr;
            const float x = lok ? sl : sr, y = rok ? sr : sl;   // one-sided fallback (:30-39)
            const float th = (go ? __builtin_fmaxf(x, y) : __builtin_fminf(x, y)) * cv.Tr;
            h[i] = col_on & (i >= b0) & (i < b1) & (m[i] >= th);
        }
    }
    bool any = false;
#pragma unroll
    for (int i = 0; i < E; ++i) any |= h[i];
    // (outside the divergent branches: the emission's ballots need every lane)
    doppler_emit<E>(o, any, [&](int i) { return h[i]; });
}

// The previous chunk's range stage inside an MTD launch: workgroup wg of the launch's nwg
// evaluates the hit regions wg, wg + nwg, ... of the previous chunk on this pipeline (the same
// tile shape, so normally exactly one), all its threads sharing a region's hits.  `skip`: the
// region-wg hits already done by a RangeJob.
__device__ __forceinline__ void prev_chunk_hits(const MtdArgs& a, int wg, int nwg, int skip) {
    const bool ref57 = a.prev_cr.ref == 5 && a.prev_cr.save == 7;
    for (int rg = wg; rg < a.prev_nregions; rg += nwg) {
        const int first = (int)threadIdx.x + (rg == wg ? skip : 0);
        if (ref57)
            cfar_hit_region<5, 7>(a.prev_rdm, a.prev_flag, a.prev_hits, a.prev_count, rg, a.prev_region, a.prev_cr,
                                  first, blockDim.x);
        else
            cfar_hit_region<0, 0>(a.prev_rdm, a.prev_flag, a.prev_hits, a.prev_count, rg, a.prev_region, a.prev_cr,
                                  first, blockDim.x);
    }
}

struct RangeHook {   // mtd_tile's after_loads(): the range job's gathers (a workgroup without a
                      // job, rj.n == 0, issues them with every lane out of range)
    RangeJob57& rj;
    const RangeSrc& s;
    static constexpr int kLoads = RangeJob57::kLoads;
    __device__ __forceinline__ void operator()() const { rj.fetch_cells(s); }
};

struct NoHook {
    static constexpr int kLoads = 0;   // vector-memory operations operator() issues
    __device__ __forceinline__ void operator()() const {}
};

// MTD tile loads by LDS-DMA (round 4; A/B in profiles/r04/ab/: c4 +5.8 %,
// c3 +1.5 %, c5 +0.4 %, outputs bit-identical): one beam, no MTI, default cache policy.  The
// tile's P rows of W complex columns (W*8 bytes each) go to LDS as 16-byte pieces
// (buffer_load_dwordx4 ... lds, no VGPR destination); a wave instruction covers 64/(W/2) whole
// rows; a row past pin loads 0 through the range check.  The range job's gathers issue behind the
// pieces and stay in flight across the barrier.  -DRSP_MTD_NO_DMA (dev-only) restores register
// loads for A/B runs.
template <int P, int BEAMS, int W>
__host__ __device__ constexpr bool kMtdDma() {
#ifndef RSP_MTD_NO_DMA
    return BEAMS == 1 && W >= 2 && W <= 128 && 64 % (W / 2) == 0;
#else
    return false;
#endif
}
typedef __attribute__((address_space(3))) void lds_void;   // an LDS-DMA destination (the MTD tiles)
template <int P, int W, int T>
__device__ __forceinline__ void mtd_dma_issue(__amdgpu_buffer_rsrc_t src, uint32_t col0, uint32_t R, unsigned char* smem,
                                              int tx) {
    constexpr int LPR = W / 2;                    // lanes per row (16 B = 2 columns each)
    constexpr int BYTES = P * W * 8;
    constexpr int NQ = BYTES / (T * 16);          // DMA instructions per thread
    static_assert(BYTES % (T * 16) == 0 && 64 % LPR == 0, "MTD DMA tiling");
    const int t = tx;
    const int wb = __builtin_amdgcn_readfirstlane(t & ~63);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int piece = q * T + t;              // 16-byte piece of the linear [P][W] image
        const int row = piece / LPR, cp = (piece % LPR) * 2;
        // (no per-lane range test: a column past R_out of a right-edge tile reads the next
        // row's first samples -- or 0 past the plane -- into an LDS column whose thread has
        // rv == false, so nothing computed from it is stored; a select here made hipcc split
        // every DMA into two exec-masked copies)
        const uint32_t vo = ((uint32_t)row * R + col0 + (uint32_t)cp) * 8u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(src, (lds_void*)(smem + (q * T + wb) * 16), 16, vo, 0, 0, 0);
    }
}

// MTD: one workgroup = W range bins x all P pulses.  Thread (c, g): range bin c of the
// tile, pulses g + G*m (m < E) -- the strided pattern of fft_reg, so the pulse-compressed
// samples load straight into registers with W-wide coalesced rows, the slow-time FFT runs
// register-resident with LDS exchanges, and |X| leaves in coalesced RDM rows.  The fftshift
// offset is 0 or P/2, a multiple of G, so bin g + G*m lands in row g + G*((m + shift/G) mod E):
// a wave-uniform rotation, and every row offset is an SGPR operand of the buffer access.
// REF > 0: Doppler CFAR specialised on the reference window; REF == 0: runtime window.
// P is the Doppler FFT length; a CPI supplies a.pin <= P pulses per beam (rows past pin are
// the zero padding of fft(x, P, 1): out of the buffer's range, they load as 0).  BEAMS == 2:
// the DMX pair -- both beams' slow-time FFTs, RDM = |X_0| + |X_1|, diff = |X_1| - |X_0|.
// Pointers of one MTD work item: the CPI's planes and the tile's hit-list region.
struct MtdTile {
    const float2* pc;      // the CPI's first PC row (beam 0); beam b starts pin rows later
    float* rdm;            // the CPI's RDM plane
    float* diff;           // the CPI's DMX difference plane, or null
    uint8_t* flagV;        // the CPI's flagV plane, or null
    uint8_t* flag;         // the CPI's flag plane, or null (no CFAR)
    uint32_t* hits;        // this tile's hit-list region (W*P entries), or null
    uint32_t* hit_count;   // where the tile's hit count goes
    uint32_t cell_base;    // hit-list number of the CPI's cell (0, 0)
    int bx;                // tile index along range
};

// fn(mm) for the thread's rows g + G*mm (mm < E) inside [lo, hi) (G a power of two; the
// arithmetic shift floors, so (x + G - 1) >> log2(G) is ceil(x / G) for negative x too)
template <int G, int E, typename F>
__device__ __forceinline__ void own_rows(int g, int lo, int hi, const F& fn) {
    constexpr int LG = __builtin_ctz(G);
    static_assert((G & (G - 1)) == 0, "G is a power of two");
    const int a0 = max(0, (lo - g + G - 1) >> LG), b0 = min(E, (hi - g + G - 1) >> LG);
#pragma clang loop unroll(disable) vectorize(disable)
    for (int mm = a0; mm < b0; ++mm) fn(mm);
}

// MTD load-phase wave priority (round 4, profiles/r04/ab/session11_mtd_prio.txt): for Doppler
// lengths P >= 256 a tile's waves run at priority 3 until the tile's loads are issued (mtd_block
// raises it, mtd_tile drops it before the FFT), so a newly resident workgroup gets its loads out
// ahead of the other tiles' compute: c4 MTD 690-707 -> 658-663 us, c4 +3.5 %, outputs identical.
// At P = 128 (c3) the same cost 1-2 %, and in the PC kernel 10 % (its rows' compute is the long
// phase), so neither has it.
#ifndef RSP_MTD_PRIO
#define RSP_MTD_PRIO 3      // (dev-only -D for A/B)
#endif
#ifndef RSP_MTD_PRIO_MINP
#define RSP_MTD_PRIO_MINP 256
#endif
constexpr int kMtdLoadPrio = RSP_MTD_PRIO, kMtdLoadPrioMinP = RSP_MTD_PRIO_MINP;

// One MTD tile: W range bins x all P pulses.
// after_loads(): called once the tile's first-beam loads are issued (RangeJob57 gathers).
template <int P, int REF, int BEAMS, typename Hook = NoHook>
__device__ __forceinline__ void mtd_tile(const MtdTile& T, const MtdArgs& a, unsigned char* smem, uint32_t* s_hits,
                                         const Hook& after_loads = Hook()) {
    using C = MtdCfg<P, BEAMS>;
    constexpr int G = C::G, E = C::E, W = C::W;
    const int tx = (int)threadIdx.x;
    if (tx == 0) *s_hits = 0u;   // published by the FFT's barriers
    const int c = tx % W, g = tx / W;
    const uint32_t R = (uint32_t)a.R_out;
    const int r = T.bx * W + c;
    const bool rv = r < (int)R;
    const uint32_t plane = (uint32_t)P * R;                     // output plane (P Doppler rows)
    const uint32_t cell = (uint32_t)g * R + (uint32_t)r;        // element (g, r) of a plane
    const int pin = a.pin;
    const uint32_t vo_in = rv ? cell * 8u : kOob;
    float2 u[E];
    float m0[BEAMS == 2 ? E : 1];     // |X_0| while beam 1 runs
    // the FFT's twiddles are loaded up front, with the tile: a twiddle load issued later (inside
    // the FFT) would make every wait for it also wait for the after_loads() gathers (vmcnt
    // counts in issue order)
    constexpr int NW = tw_regs<P, E>() > 0 ? tw_regs<P, E>() : 1;
    float2 tw[NW];
    tw_preload<P, G, 1, E, 0, NW>(tw, g, a.tw);
#pragma unroll
    for (int b = 0; b < BEAMS; ++b) {
        const auto src = buf_rsrc(T.pc + (size_t)b * pin * R, (uint32_t)pin * R * 8u);
        if (a.mti_lag > 0) {   // fused MTI (wave-uniform): pulse p = PC(p + lag) - PC(p), 0 past pin - lag
            const int lag = a.mti_lag;
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const float2 v0 = buf_ld_f2(src, vo_in, (uint32_t)(G * m) * R * 8u);
                const float2 v1 = buf_ld_f2(src, vo_in, (uint32_t)(G * m + lag) * R * 8u);
                const float w = g + G * m + lag < pin ? a.win[g + G * m] : 0.f;
                u[m] = make_float2((v1.x - v0.x) * w, (v1.y - v0.y) * w);
            }
        } else if constexpr (kMtdDma<P, BEAMS, W>()) {
            // the tile's P rows x W columns land in LDS by DMA (row-major [p][c], linear), then
            // thread (c, g) reads its strided pulses; the range job's gathers issue behind the
            // DMA and stay in flight across the barrier (a counted vmcnt, a raw s_barrier)
            float wv[E];
#pragma unroll
            for (int m = 0; m < E; ++m) wv[m] = a.win[g + G * m];
            mtd_dma_issue<P, W, C::T>(src, (uint32_t)(T.bx * W), R, smem, tx);
            // (a compiler barrier: the range gathers below must issue after every DMA piece, or
            // the counted vmcnt would not cover the pieces -- hipcc interleaved them otherwise)
            asm volatile("" ::: "memory");
            // (one path per kernel instance -- the range job is a template choice, not a runtime
            // branch: where a job / no-job branch merged, hipcc's waitcnt pass, which cannot read
            // an asm wait, counted from the no-job side and made the window multiply wait for
            // most gathers).  The weights and twiddles are older than the gathers, so the wait
            // covers them; redefined behind it, no later use of them waits for the gathers, which
            // stay in flight through the FFT and the Doppler CFAR (lds_barrier).
            after_loads();
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(Hook::kLoads) : "memory");
#pragma unroll
            for (int m = 0; m < E; ++m) asm volatile("" : "+v"(wv[m]));
#pragma unroll
            for (int i = 0; i < NW; ++i) asm volatile("" : "+v"(tw[i]));
            // (the barrier as asm with a memory clobber: __builtin_amdgcn_s_barrier touches no
            // memory at the IR level, so nothing would keep the LDS reads below it)
            asm volatile("s_barrier" ::: "memory");
            const float2* l = reinterpret_cast<const float2*>(smem);
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const float2 v = l[(g + G * m) * W + c];
                u[m] = make_float2(v.x * wv[m], v.y * wv[m]);
            }
        } else {
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const float2 v = buf_ld_f2(src, vo_in, (uint32_t)(G * m) * R * 8u);
                const float w = a.win[g + G * m];
                u[m] = make_float2(v.x * w, v.y * w);
            }
        }
        if (b == 0 && !(kMtdDma<P, BEAMS, W>() && a.mti_lag <= 0)) after_loads();
        RSP_STAMP(1, 1, true);
        if constexpr (P >= kMtdLoadPrioMinP) __builtin_amdgcn_s_setprio(0);   // the tile's loads are out
        fft_reg_w<P, G, 1, E, 0, NW>(u, reinterpret_cast<float2*>(smem) + c * C::SLOT, g, tw);
        RSP_STAMP(1, 2, false);
        if constexpr (BEAMS == 2) {
            if (b == 0) {
#pragma unroll
                for (int m = 0; m < E; ++m) m0[m] = __builtin_amdgcn_sqrtf(fmaf(u[m].x, u[m].x, u[m].y * u[m].y));
            }
        }
    }

    // The flag plane's zero background for this tile (range stage on: the 1s come later from
    // the hit list): W columns x P rows, one 16-byte store per row segment, issued while the
    // FFT runs -- instead of a byte store per cell in the Doppler epilogue.
    bool bg_done = false;
    if constexpr (W % 16 == 0) {
        if (T.flag && a.cv.enabled && a.rflag && a.flag_zero && (R % 16u) == 0u) {
            typedef int v4i __attribute__((ext_vector_type(4)));
            const auto fz = buf_rsrc(T.flag, plane);
            constexpr int SEG = W / 16;
            for (int i = tx; i < P * SEG; i += C::T) {
                const int c0 = T.bx * W + (i % SEG) * 16;
                if (c0 < (int)R)
                    __builtin_amdgcn_raw_buffer_store_b128(v4i{0, 0, 0, 0}, fz, (uint32_t)(i / SEG) * R + (uint32_t)c0,
                                                           0u, 0);
            }
            bg_done = true;
        }
    }

    const auto dst = buf_rsrc(T.rdm, plane * 4u);
    const bool want_diff = BEAMS == 2 && T.diff != nullptr;
    const auto dfr = buf_rsrc(want_diff ? T.diff : nullptr, want_diff ? plane * 4u : 0u);
    const uint32_t vo_out = rv ? cell * 4u : kOob;
    const int srot = a.shift / G;
    float mg[E];
#pragma unroll
    for (int m = 0; m < E; ++m) {
        int mm = m + srot;                // fftshift: bin g + G*m -> row g + G*mm
        if (mm >= E) mm -= E;
        float x = __builtin_amdgcn_sqrtf(fmaf(u[m].x, u[m].x, u[m].y * u[m].y));
        if constexpr (BEAMS == 2) {
            if (want_diff) buf_st_f(x - m0[m], dfr, vo_out, (uint32_t)(G * mm) * R * 4u);   // |R| - |L|
            x += m0[m];                                                                      // |L| + |R|
        }
        mg[m] = x;
        buf_st_f_stream(x, dst, vo_out, (uint32_t)(G * mm) * R * 4u);
    }
    // fun_0v_pressing's zeroed rows [z_lo, z_hi) (the DMX zeroSetFlagMTD band wraps through row
    // 0: rows [0, z_hi - P) too), as a second store of 0 to the few of the thread's rows inside
    // the band -- the same thread's later store to the same address wins -- instead of a
    // compare-select on every row (one or two rows per thread; 4 VALU per row saved)
    const int zw = a.z_hi > P ? a.z_hi - P : 0;
    auto zero_rdm = [&](int mm) {   // (mm is per lane: the row offset goes in the VGPR offset)
        const uint32_t vz = rv ? (cell + (uint32_t)(G * mm) * R) * 4u : kOob;
        buf_st_f_stream(0.f, dst, vz, 0u);
    };
    own_rows<G, E>(g, a.z_lo, a.z_hi, zero_rdm);
    own_rows<G, E>(g, 0, zw, zero_rdm);
    RSP_STAMP(1, 3, false);
    if (!a.cv.enabled) return;
    lds_barrier();  // the FFT exchange slots are free from here on
    float* mag = REF > 0 ? reinterpret_cast<float*>(smem) + c * C::MS2 + C::SPAD
                         : reinterpret_cast<float*>(smem) + c * C::MS;
#pragma unroll
    for (int m = 0; m < E; ++m) {
        int mm = m + srot;
        if (mm >= E) mm -= E;
        mag[g + G * mm] = mg[m];
    }
    // the CFAR input's zero rows (main_cfar.m:90-91) and the RDM's band, by the same second
    // write of 0 (LDS writes of one thread land in order)
    auto zero_mag = [&](int mm) { mag[g + G * mm] = 0.f; };
    own_rows<G, E>(g, a.z_lo, a.z_hi, zero_mag);
    own_rows<G, E>(g, 0, zw, zero_mag);
    own_rows<G, E>(g, a.cv.cz_lo, a.cv.cz_hi, zero_mag);
    lds_barrier();

    const int v0 = cfar_run<G, W>(g) * E;   // this thread's run of Doppler rows
    const bool col_on = rv && in_segs(r, a.cv.nseg, a.cv.seg_lo, a.cv.seg_hi);
    DopplerOut o;
    o.want_fv = T.flagV != nullptr;
    o.fused = T.flag != nullptr;
    o.rflag = a.rflag != 0;
    o.zero_bg = a.flag_zero != 0 && !bg_done;
    o.fv = buf_rsrc(o.want_fv ? T.flagV : nullptr, o.want_fv ? plane : 0u);
    o.fl = buf_rsrc(o.fused ? T.flag : nullptr, o.fused ? plane : 0u);
    o.vo = rv ? (uint32_t)v0 * R + (uint32_t)r : kOob;
    o.R = R;
    o.hits = T.hits;
    o.lds_count = s_hits;
    o.cell0 = T.cell_base + (uint32_t)v0 * R + (uint32_t)r;
    if constexpr (REF > 0) {
        doppler_cfar_fixed<P, REF, BEAMS>(mag, a.cv, col_on, v0, o);
    } else {
        float* sums = reinterpret_cast<float*>(smem) + W * C::MS + c * C::SMS + C::SPAD;
        doppler_sums(mag, sums, P, a.cv.ref, v0, v0 + E);
        lds_barrier();
        doppler_flags<E>(mag, sums, a.cv, col_on, v0, v0 + E, o);
    }
    RSP_STAMP(1, 4, false);
    if (o.fused && o.rflag) {
        lds_barrier();
        if (tx == 0) *T.hit_count = *s_hits;
    }
}

// MTD: one workgroup = W range bins x all P pulses.  Thread (c, g): range bin c of the
// tile, pulses g + G*m (m < E) -- the strided pattern of fft_reg, so the pulse-compressed
// samples load straight into registers with W-wide coalesced rows, the slow-time FFT runs
// register-resident with LDS exchanges, and |X| leaves in coalesced RDM rows.  The fftshift
// offset is 0 or P/2, a multiple of G, so bin g + G*m lands in row g + G*((m + shift/G) mod E):
// a wave-uniform rotation, and every row offset is an SGPR operand of the buffer access.
// REF > 0: Doppler CFAR specialised on the reference window; REF == 0: runtime window.
// P is the Doppler FFT length; a CPI supplies a.pin <= P pulses per beam (rows past pin are
// the zero padding of fft(x, P, 1): out of the buffer's range, they load as 0).  BEAMS == 2:
// the DMX pair -- both beams' slow-time FFTs, RDM = |X_0| + |X_1|, diff = |X_1| - |X_0|.
// One MTD workgroup: tile bx (of gx along range) of launch CPI by (of gy); smem / s_hits: the
// workgroup's dynamic LDS and hit counter.
template <int P, int REF, int BEAMS, bool JOB>
__device__ __forceinline__ void mtd_block(const float2* __restrict__ pc, float* __restrict__ rdm,
                                          uint8_t* __restrict__ flagV, const MtdArgs& a, int bx, int by, int gx, int gy,
                                          unsigned char* smem, uint32_t* s_hits) {
    using C = MtdCfg<P, BEAMS>;
    const size_t cpi = (size_t)by;
    const size_t R = (size_t)a.R_out;
    const size_t plane = (size_t)P * R;
    size_t row0 = cpi * (size_t)a.pin * BEAMS;                   // first PC row of this CPI
    if (a.nwin > 0) row0 = (cpi / a.nwin) * (size_t)a.pin + a.win_start[cpi % a.nwin];
    const uint32_t wg = (uint32_t)by * (uint32_t)gx + (uint32_t)bx;
    MtdTile T;
    T.pc = pc + row0 * R;
    T.rdm = rdm + cpi * plane;
    T.diff = (BEAMS == 2 && a.diff) ? a.diff + cpi * plane : nullptr;
    T.flagV = flagV ? flagV + cpi * plane : nullptr;
    T.flag = a.flag ? a.flag + cpi * plane : nullptr;
    T.hits = a.hits ? a.hits + (size_t)wg * (C::W * P) : nullptr;
    T.hit_count = a.hit_count ? a.hit_count + wg : nullptr;
    T.cell_base = (uint32_t)(cpi * plane) + a.cell_off;
    T.bx = bx;
    if constexpr (C::W < 32) {   // 8 consecutive tiles on one XCD (workgroup x goes to XCD x % 8):
        // their partial RDM / flag row segments (W = 16: 64-B RDM and 16-B flag segments) meet
        // in one L2 and leave it as whole lines -- 8 tiles make the flag segments whole 128-B
        // lines too (c4 MTD 419 -> 397 us per launch, c4 +4.7 %; c5 neutral; 4 tiles: c5 +1.5-2 %
        // over none); 4 tiles when the row's tile count is not a multiple of 64.  (At W = 32 the
        // RDM segments are whole lines and grouping cost c3's MTD 3 %.)
        const int x = bx;
        if (gx % 64 == 0) T.bx = (x / 64) * 64 + (x % 8) * 8 + (x / 8) % 8;
        else if (gx % 32 == 0) T.bx = (x / 32) * 32 + (x % 8) * 4 + (x / 8) % 4;
    }
    const int nwg = gx * gy;
    // one instance of the tile (the kernel's code stays ~half the size: it shares the
    // instruction cache with the PC kernel of the other pipeline); the range job is runtime-
    // guarded -- with n == 0 its hook and finish() return at once
    const bool job = JOB && a.prev_nregions > 0 && a.prev_cr.ref == 5 && a.prev_cr.save == 7 && (int)wg < a.prev_nregions &&
                     (uint64_t)a.prev_nregions * (uint64_t)a.prev_region < (uint64_t)(kOob / 4u);
    RangeJob57 rj;
    const RangeSrc rs = RangeSrc::of(a);
    RSP_STAMP(1, 0, false);
    if constexpr (P >= kMtdLoadPrioMinP) __builtin_amdgcn_s_setprio(kMtdLoadPrio);
    RSP_STAMP_RT(1, 8);
    if (job) rj.fetch_idx(rs, (int)wg);
    if constexpr (JOB) mtd_tile<P, REF, BEAMS>(T, a, smem, s_hits, RangeHook{rj, rs});
    else mtd_tile<P, REF, BEAMS>(T, a, smem, s_hits, NoHook{});
    RSP_STAMP(1, 5, false);
    rj.finish(rs);
    RSP_STAMP(1, 6, false);
    if (job ? (rj.n > blockDim.x || a.prev_nregions > nwg) : a.prev_nregions > 0)
        prev_chunk_hits(a, (int)wg, nwg, job ? (int)blockDim.x : 0);
    RSP_STAMP(1, 7, true);
    RSP_STAMP_RT(1, 9);
}

// JOB: this launch carries the previous chunk's range stage for the reference's window (the
// RangeJob57 gathers ride on the tile load); otherwise prev_chunk_hits (if any) runs after the tile.
template <int P, int REF, int BEAMS, bool JOB>
__global__ __launch_bounds__((MtdCfg<P, BEAMS>::T), (MtdCfg<P, BEAMS>::WPE)) void mtd_kernel(const float2* __restrict__ pc,
                                                     float* __restrict__ rdm,
                                                     uint8_t* __restrict__ flagV, MtdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_hits;
    mtd_block<P, REF, BEAMS, JOB>(pc, rdm, flagV, a, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x, (int)gridDim.y,
                                  smem, &s_hits);
}

// Slow-time DFT for a pulse count without a radix plan (the v2 native P = 332 = 4*83,
// MTD/main_produce_dataset_win_xzr_v2.m:31) by Bluestein's identity:
//   X[k] = c[k] sum_n (x[n] w[n] c[n]) conj(c[k-n]),   c[n] = exp(-j pi n^2 / P),
// a circular convolution of length NF >= 2P - 1 (power of two): FFT, multiply by the chirp's
// spectrum, FFT again (the inverse as conj(FFT(conj))).  |c[k]| = 1, so the magnitude
// needs no final chirp.  Bins k < P are kept; fftshift / 0-v / Doppler CFAR as mtd_kernel
// (runtime CFAR window), with per-element row offsets (P is not a multiple of G).
template <int NF>
__global__ __launch_bounds__(MtdCfg<NF>::T) void mtd_bluestein_kernel(const float2* __restrict__ pc,
                                                               float* __restrict__ rdm,
                                                               uint8_t* __restrict__ flagV, MtdArgs a) {
    using C = MtdCfg<NF>;
    constexpr int G = C::G, E = C::E, W = C::W;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_hits;
    if (threadIdx.x == 0) s_hits = 0u;
    const int c = threadIdx.x % W, g = threadIdx.x / W;
    const size_t cpi = blockIdx.y;
    const uint32_t R = (uint32_t)a.R_out;
    const int r = blockIdx.x * W + c;
    const bool rv = r < (int)R;
    const int P = a.pin;
    const uint32_t plane = (uint32_t)P * R;
    size_t row0 = cpi * (size_t)P;
    if (a.nwin > 0) row0 = (cpi / a.nwin) * (size_t)P + a.win_start[cpi % a.nwin];
    const auto src = buf_rsrc(pc + row0 * R, plane * 8u);           // rows >= P load as 0
    const uint32_t vo_in = rv ? ((uint32_t)g * R + (uint32_t)r) * 8u : kOob;
    float2 u[E];
    if (a.mti_lag > 0) {   // fused MTI, as mtd_tile
        const int lag = a.mti_lag;
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const float2 v0 = buf_ld_f2(src, vo_in, (uint32_t)(G * m) * R * 8u);
            const float2 v1 = buf_ld_f2(src, vo_in, (uint32_t)(G * m + lag) * R * 8u);
            const float2 d = g + G * m + lag < P ? make_float2(v1.x - v0.x, v1.y - v0.y) : make_float2(0.f, 0.f);
            u[m] = cmul(d, a.bwc[g + G * m]);
        }
    } else {
#pragma unroll
        for (int m = 0; m < E; ++m)
            u[m] = cmul(buf_ld_f2(src, vo_in, (uint32_t)(G * m) * R * 8u), a.bwc[g + G * m]);
    }
    float2* slot = reinterpret_cast<float2*>(smem) + c * C::SLOT;
    fft_reg<NF, G, 1, E>(u, slot, g, a.tw);
#pragma unroll
    for (int m = 0; m < E; ++m) u[m] = cmul_conj(u[m], a.bspec[g + G * m]);   // conj(A .* B), 1/NF in B
    fft_reg<NF, G, 1, E>(u, slot, g, a.tw);                                  // conj of the convolution

    const auto dst = buf_rsrc(rdm + cpi * plane, plane * 4u);
    float mg[E];
    int vr[E];
    const int zw = a.z_hi > P ? a.z_hi - P : 0;   // the zero_ends band wraps through row 0, as in mtd_tile
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int k = g + G * m;                   // Doppler bin
        int v = k + a.shift;                       // fftshift: out[v] = X[(v - shift) mod P]
        if (v >= P) v -= P;
        float x = __builtin_amdgcn_sqrtf(fmaf(u[m].x, u[m].x, u[m].y * u[m].y));
        if ((v >= a.z_lo && v < a.z_hi) || v < zw) x = 0.f;   // fun_0v_pressing / zero_ends
        mg[m] = x;
        vr[m] = k < P ? v : -1;
        if (k < P) buf_st_f(x, dst, rv ? ((uint32_t)v * R + (uint32_t)r) * 4u : kOob, 0u);
    }
    if (!a.cv.enabled) return;   // (no CFAR: no range stage pending either)
    __syncthreads();  // the FFT exchange slots are free from here on
    float* mag = reinterpret_cast<float*>(smem) + c * C::MS;
#pragma unroll
    for (int m = 0; m < E; ++m)
        if (vr[m] >= 0) mag[vr[m]] = (vr[m] >= a.cv.cz_lo && vr[m] < a.cv.cz_hi) ? 0.f : mg[m];
    __syncthreads();
    const int v0 = g * E, v1 = v0 + E < P ? v0 + E : P;    // this thread's run of Doppler rows
    const bool col_on = rv && in_segs(r, a.cv.nseg, a.cv.seg_lo, a.cv.seg_hi);
    DopplerOut o;
    o.want_fv = flagV != nullptr;
    o.fused = a.flag != nullptr;
    o.rflag = a.rflag != 0;
    o.zero_bg = a.flag_zero != 0;
    o.fv = buf_rsrc(o.want_fv ? flagV + cpi * plane : nullptr, o.want_fv ? plane : 0u);
    o.fl = buf_rsrc(o.fused ? a.flag + cpi * plane : nullptr, o.fused ? plane : 0u);
    o.vo = (rv && v0 < P) ? (uint32_t)v0 * R + (uint32_t)r : kOob;
    o.R = R;
    const uint32_t wg = blockIdx.y * gridDim.x + blockIdx.x;
    o.hits = a.hits ? a.hits + (size_t)wg * ((size_t)W * P) : nullptr;
    o.lds_count = &s_hits;
    o.cell0 = (uint32_t)cpi * plane + a.cell_off + (uint32_t)v0 * R + (uint32_t)r;
    float* sums = reinterpret_cast<float*>(smem) + W * C::MS + c * C::SMS + C::SPAD;
    doppler_sums(mag, sums, P, a.cv.ref, v0, v1);
    __syncthreads();
    doppler_flags<E>(mag, sums, a.cv, col_on, v0, v1, o);
    if (o.fused && o.rflag) {
        __syncthreads();
        if (threadIdx.x == 0) a.hit_count[wg] = s_hits;
    }
    if (a.prev_nregions > 0) prev_chunk_hits(a, (int)wg, (int)(gridDim.x * gridDim.y), 0);
}

template <int NF>
static hipError_t launch_mtd_bluestein(const float2* pc, float* rdm, uint8_t* flagV, int ncpi, const MtdArgs& a,
                                       hipStream_t s) {
    using C = MtdCfg<NF>;
    if (a.pin < 2 || 2 * a.pin - 1 > NF || a.beams != 1 || a.shift < 0 || a.shift >= a.pin) return hipErrorInvalidValue;
    if (a.cv.enabled && a.cv.save + a.cv.ref + 2 > C::SPAD) return hipErrorInvalidValue;
    if ((uint64_t)a.pin * a.R_out * 8 >= (uint64_t)kOob) return hipErrorInvalidValue;
    static LaunchOnce once;
    hipError_t e = lds_attr(once, (const void*)mtd_bluestein_kernel<NF>, C::lds);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)((a.R_out + C::W - 1) / C::W), (unsigned)ncpi),
        block(C::T);
    hipLaunchKernelGGL((mtd_bluestein_kernel<NF>), grid, block, C::lds, s, pc, rdm, flagV, a);
    return hipGetLastError();
}

int mtd_bluestein_nf(int P) {
    int nf = 64;
    while (nf < 2 * P - 1) nf <<= 1;
    return nf <= 2048 ? nf : 0;
}

// The Doppler stage compiled into mtd_kernel<P, 5, ...> (the reference's 5 + 7 window); any other
// window runs the runtime-window instance <P, 0, ...>.  Bluestein tiles always take the runtime form.
bool mtd_window_compiled(const MtdArgs& a) { return a.bnf == 0 && a.cv.enabled && a.cv.ref == 5 && a.cv.save == 7; }

// The in-launch range job (RangeJob57) only in the compiled-window instance and for the reference's
// range window; any other previous-chunk range stage runs as prev_chunk_hits in the no-job instance.
bool mtd_range_job57(const MtdArgs& a) {
    return mtd_window_compiled(a) && a.prev_nregions > 0 && a.prev_cr.ref == 5 && a.prev_cr.save == 7 &&
           (uint64_t)a.prev_nregions * (uint64_t)a.prev_region < (uint64_t)(kOob / 4u);
}

template <int P, int REF, int BEAMS>
static hipError_t launch_mtd_pr(const float2* pc, float* rdm, uint8_t* flagV, int ncpi,
                                const MtdArgs& a, hipStream_t s) {
    using C = MtdCfg<P, BEAMS>;
    constexpr size_t lds = C::template lds_for<REF>();
    static LaunchOnce once, once_job;
    dim3 grid((unsigned)((a.R_out + C::W - 1) / C::W), (unsigned)ncpi),
        block(C::T);
    const bool job = REF > 0 && mtd_range_job57(a);
    if constexpr (REF > 0) {
        if (job) {
            hipError_t e = lds_attr(once_job, (const void*)mtd_kernel<P, REF, BEAMS, true>, lds);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL((mtd_kernel<P, REF, BEAMS, true>), grid, block, lds, s, pc, rdm, flagV, a);
            return hipGetLastError();
        }
    }
    hipError_t e = lds_attr(once, (const void*)mtd_kernel<P, REF, BEAMS, false>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((mtd_kernel<P, REF, BEAMS, false>), grid, block, lds, s, pc, rdm, flagV, a);
    return hipGetLastError();
}

template <int P, int BEAMS = 1>
static hipError_t launch_mtd_p(const float2* pc, float* rdm, uint8_t* flagV, int ncpi,
                               const MtdArgs& a, hipStream_t s) {
    using C = MtdCfg<P, BEAMS>;
    // shift is 0 or floor(P/2) = G*E/2; the row rotation needs it to be a multiple of G,
    // and the padded sums column needs save + ref + 2 <= SPAD
    if (a.shift % C::G != 0 || a.shift < 0 || a.shift >= P) return hipErrorInvalidValue;
    if (a.cv.enabled && a.cv.save + a.cv.ref + 2 > C::SPAD) return hipErrorInvalidValue;
    if ((uint64_t)P * a.R_out * 8 >= (uint64_t)kOob) return hipErrorInvalidValue;
    if (a.pin < 1 || a.pin > P || a.beams != BEAMS) return hipErrorInvalidValue;
    if (mtd_window_compiled(a)) return launch_mtd_pr<P, 5, BEAMS>(pc, rdm, flagV, ncpi, a, s);
    return launch_mtd_pr<P, 0, BEAMS>(pc, rdm, flagV, ncpi, a, s);
}

// The tile of one MTD workgroup: W range bins by T threads (MtdCfg of the instance launch_mtd runs;
// Bluestein: of its NF-point transform).  false: no instance for (P, beams).
template <int P, int BEAMS>
static void mtd_geometry_p(int* W, int* T) {
    using C = MtdCfg<P, BEAMS>;
    *W = C::W;
    *T = C::T;
}

bool mtd_geometry(int P, int beams, int* W, int* T) {
    *W = 0;
    *T = 0;
    if (beams == 1 && !mtd_size_supported(P, 1)) {   // Bluestein: NF-point tiles, P rows kept
        switch (mtd_bluestein_nf(P)) {
#define RSP_MB(nf) case nf: mtd_geometry_p<nf, 1>(W, T); break;
            RSP_MB(64) RSP_MB(128) RSP_MB(256) RSP_MB(512) RSP_MB(1024) RSP_MB(2048)
#undef RSP_MB
            default: break;
        }
        return *W > 0;
    }
    if (beams == 2) {
        switch (P) {
            case 512: mtd_geometry_p<512, 2>(W, T); break;
            case 1024: mtd_geometry_p<1024, 2>(W, T); break;
            case 2048: mtd_geometry_p<2048, 2>(W, T); break;
            default: break;
        }
        return *W > 0;
    }
    switch (P) {
#define RSP_MR(p) case p: mtd_geometry_p<p, 1>(W, T); break;
        RSP_MR(16) RSP_MR(32) RSP_MR(64) RSP_MR(128) RSP_MR(256) RSP_MR(512) RSP_MR(1024)
        RSP_MR(2048) RSP_MR(48) RSP_MR(96) RSP_MR(192) RSP_MR(384) RSP_MR(768) RSP_MR(1536)
#undef RSP_MR
        default: break;
    }
    return *W > 0;
}

// Hit-list regions of one MTD launch: one per workgroup (tile of W range bins), W * P
// entries each -- the tile's own cells, so a region can never overflow.
void mtd_regions(int P, int R_out, int ncpi, int* nregions, int* region, int beams) {
    *nregions = 0;
    *region = 0;
    int W = 0, T = 0;
    if (!mtd_geometry(P, beams, &W, &T)) return;
    *nregions = ((R_out + W - 1) / W) * ncpi;
    *region = W * P;
}

bool mtd_size_supported(int P, int beams) {
    if (beams == 2) return P == 512 || P == 1024 || P == 2048;   // the DMX pair (mtd_FFT_num 2048)
    if (beams != 1) return false;
    switch (P) {
        case 16: case 32: case 64: case 128: case 256: case 512: case 1024: case 2048:
        case 48: case 96: case 192: case 384: case 768: case 1536:
            return true;
        default:
            return false;
    }
}

hipError_t launch_mtd(const float2* pc, float* rdm, uint8_t* flagV, int ncpi, const MtdArgs& a,
                      hipStream_t s) {
    if (ncpi <= 0) return hipSuccess;
    if (a.bnf > 0) {
        switch (a.bnf) {
            case 64: return launch_mtd_bluestein<64>(pc, rdm, flagV, ncpi, a, s);
            case 128: return launch_mtd_bluestein<128>(pc, rdm, flagV, ncpi, a, s);
            case 256: return launch_mtd_bluestein<256>(pc, rdm, flagV, ncpi, a, s);
            case 512: return launch_mtd_bluestein<512>(pc, rdm, flagV, ncpi, a, s);
            case 1024: return launch_mtd_bluestein<1024>(pc, rdm, flagV, ncpi, a, s);
            case 2048: return launch_mtd_bluestein<2048>(pc, rdm, flagV, ncpi, a, s);
            default: return hipErrorInvalidValue;
        }
    }
    if (a.beams == 2) {
        switch (a.P) {
            case 512: return launch_mtd_p<512, 2>(pc, rdm, flagV, ncpi, a, s);
            case 1024: return launch_mtd_p<1024, 2>(pc, rdm, flagV, ncpi, a, s);
            case 2048: return launch_mtd_p<2048, 2>(pc, rdm, flagV, ncpi, a, s);
            default: return hipErrorInvalidValue;
        }
    }
    switch (a.P) {
        case 16: return launch_mtd_p<16>(pc, rdm, flagV, ncpi, a, s);
        case 32: return launch_mtd_p<32>(pc, rdm, flagV, ncpi, a, s);
        case 64: return launch_mtd_p<64>(pc, rdm, flagV, ncpi, a, s);
        case 128: return launch_mtd_p<128>(pc, rdm, flagV, ncpi, a, s);
        case 256: return launch_mtd_p<256>(pc, rdm, flagV, ncpi, a, s);
        case 512: return launch_mtd_p<512>(pc, rdm, flagV, ncpi, a, s);
        case 1024: return launch_mtd_p<1024>(pc, rdm, flagV, ncpi, a, s);
        case 2048: return launch_mtd_p<2048>(pc, rdm, flagV, ncpi, a, s);
        case 48: return launch_mtd_p<48>(pc, rdm, flagV, ncpi, a, s);
        case 96: return launch_mtd_p<96>(pc, rdm, flagV, ncpi, a, s);
        case 192: return launch_mtd_p<192>(pc, rdm, flagV, ncpi, a, s);
        case 384: return launch_mtd_p<384>(pc, rdm, flagV, ncpi, a, s);
        case 768: return launch_mtd_p<768>(pc, rdm, flagV, ncpi, a, s);
        case 1536: return launch_mtd_p<1536>(pc, rdm, flagV, ncpi, a, s);
        default: return hipErrorInvalidValue;
    }
}

#ifdef RSP_DIAG_STAMPS
int diag_fetch_mtd(uint64_t* host, int64_t n) { return diag_fetch(host, n); }
#endif

// (Round 5's persistent one-launch PC -> MTD dataflow, flow_kernel / rsp_set_flow, measured 82 %
// of the chunked chain at c3 and left the product in round 6: DESIGN.md §7c / §7d; its source is
// in the history, commit e3a7a73.  Round 6's split form -- a PC-only and an MTD-only persistent
// kernel on CU-masked streams -- measured 75.6 % (profiles/r06/flow2/ab_record.txt, commit
// d7d9bbe).  Those kernels instantiated sc1 cache-policy and opaque-thread-index variants of the PC
// row, the MTD tile and the range job, and the in-launch hand-off accessors of rsp_buf.h; all of
// them are in those commits too.)

}  // namespace rsp
