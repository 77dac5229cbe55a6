// rsp_ingest_legacy.hip -- the legacy two-beam 24-bit PRT records for gfx950: the decode of
// frameDataRead_A (MatlabProcess_xuzerui/frameDataRead_A_xzr.m:53-148, Show_Read.m:49-142)
// straight into the [beam][prt][sample] complex64 planes that the PC -> MTD chain reads.
//
// Record (little-endian, rec = 28 + 12 * point_prt + 8 bytes, always a multiple of 4):
//   0-3    two uint16 sync words (0xA5A5), read and never checked by the reference
//   4-7    frameInd = u16[2] * 2^16 + u16[3] (high word first)
//   8-9    modFlag, 10 beamPosNum, 11 beamNums, 12-13 freInd, 14-15 prtInd
//   16-25  skipped
//   26-27  angleCode = (b26 + b27 * 2^7) * 360 / 16384   (2^7 as written, :75-77)
//   28...  point_prt groups of 12 bytes [Ql Il Qr Ir](high) [Ql Il Qr Ir](mid) [Ql Il Qr Ir](low)
//   last 8 tail, skipped
// A group read as three dwords is one dword of high bytes, one of middle bytes and one of low
// bytes with the four channels side by side, so channel k is byte k of each dword.
// Sample: v = hi * 2^16 + mid * 2^8 + lo, and v - 2^24 if v > 2^23 (:112-129): 0x800000 stays
// +8388608.  Every value has magnitude <= 2^23 and is exact in fp32.
//
// One launch decodes every row (frame x PRT): a block per (256-sample tile, PRT, frame), one
// thread per sample.  A lane reads its group's three dwords (a wave: 768 contiguous bytes, every
// byte of every line used) and stores one float2 to each beam's row (512 contiguous bytes per
// wave and plane; rows are 8-byte aligned only, point_prt being odd in the real geometry).  The
// record size is fixed, so the host knows from the byte count alone which rows are whole: there
// is no check kernel, and rows from the first cut one on are written as zeros.  Lane 0 of a
// row's first tile writes the row's head fields, angle and status.  The work is memory-bound:
// 12 B read and 16 B written per sample.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rsp.h"
#include "rsp_internal.h"

namespace rsp {

constexpr int kLegacyTile = 256;

// hi * 2^16 + mid * 2^8 + lo of byte k of the three dwords, with the reference's sign rule
template <int K>
__device__ __forceinline__ float legacy_sample(uint32_t hi, uint32_t mid, uint32_t lo) {
    const uint32_t v = (((hi >> (8 * K)) & 0xffu) << 16) | (((mid >> (8 * K)) & 0xffu) << 8) | ((lo >> (8 * K)) & 0xffu);
    return (float)(v > 0x800000u ? (int32_t)v - (1 << 24) : (int32_t)v);   // > 2^23, not >= (:112)
}

__global__ __launch_bounds__(kLegacyTile) void ingest_legacy_kernel(const uint8_t* __restrict__ stream, LegacyIngestArgs a,
                                                                     float2* __restrict__ out, double* __restrict__ angle,
                                                                     int32_t* __restrict__ head,
                                                                     int32_t* __restrict__ status) {
    const int prt = blockIdx.y, f = blockIdx.z;
    const int64_t row = (int64_t)f * a.prt_num + prt;
    const int s = blockIdx.x * kLegacyTile + threadIdx.x;
    const bool decoded = row < a.rows_decoded;   // (block-uniform) the whole record but its tail lies inside nbytes
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(stream + row * a.rec_bytes);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int32_t h[RSP_LEGACY_HEAD_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0};
        double ang = 0.0;
        if (decoded) {
            const uint32_t w0 = rec[0], w1 = rec[1], w2 = rec[2], w3 = rec[3], w6 = rec[6];
            h[0] = (int32_t)((w1 << 16) | (w1 >> 16));   // frameInd1 * 2^16 + frameInd2 (:60-62)
            h[1] = (int32_t)(w2 & 0xffffu);              // modFlag
            h[2] = (int32_t)((w2 >> 16) & 0xffu);        // beamPosNum
            h[3] = (int32_t)(w2 >> 24);                  // beamNums
            h[4] = (int32_t)(w3 & 0xffffu);              // freInd
            h[5] = (int32_t)(w3 >> 16);                  // prtInd
            h[6] = w0 == 0xA5A5A5A5u ? 1 : 0;            // sync_ok (the reference never checks)
            // (angleCode1 + angleCode2 * 2^7) * 360 / 16384: an integer below 2^24 over a power of two
            ang = (double)((((w6 >> 16) & 0xffu) + ((w6 >> 24) << 7)) * 360u) / 16384.0;
        }
        if (head) {
#pragma unroll
            for (int k = 0; k < RSP_LEGACY_HEAD_FIELDS; ++k) head[row * RSP_LEGACY_HEAD_FIELDS + k] = h[k];
        }
        if (angle) angle[row] = ang;
        // the record's end against the byte count: whole, tail cut (still decoded), or cut
        const int64_t end = (row + 1) * a.rec_bytes;
        status[row] = end <= a.nbytes ? RSP_PRT_OK : decoded ? RSP_PRT_TAIL_TRUNCATED : RSP_PRT_TRUNCATED;
        if (row == 0) status[a.rows] = (int32_t)a.rows_decoded;
    }
    if (s >= a.point_prt) return;
    float2 left = make_float2(0.f, 0.f), right = make_float2(0.f, 0.f);
    if (decoded) {
        const uint32_t* g = rec + 7 + 3 * (size_t)s;   // payload at byte 28
        const uint32_t hi = g[0], mid = g[1], lo = g[2];
        left = make_float2(legacy_sample<1>(hi, mid, lo), legacy_sample<0>(hi, mid, lo));    // I_l + j Q_l
        right = make_float2(legacy_sample<3>(hi, mid, lo), legacy_sample<2>(hi, mid, lo));   // I_r + j Q_r
    }
    float2* o = out + (int64_t)f * a.frame_stride + (int64_t)prt * a.point_prt + s;
    o[0] = left;
    o[a.beam_stride] = right;
}

hipError_t launch_ingest_legacy(const uint8_t* stream, const LegacyIngestArgs& a, float2* out, double* angle,
                                int32_t* head, int32_t* status, hipStream_t s) {
    const dim3 grid((unsigned)((a.point_prt + kLegacyTile - 1) / kLegacyTile), (unsigned)a.prt_num, (unsigned)a.nframes);
    hipLaunchKernelGGL(ingest_legacy_kernel, grid, dim3(kLegacyTile), 0, s, stream, a, out, angle, head, status);
    return hipGetLastError();
}

}  // namespace rsp
