// rsp_hostplan.h -- the integer planning of the host-buffer entry points (rsp_host.cpp): how a
// transfer is cut into ring pieces, a batch into host chunks, and a one-chunk call's input and
// outputs into the pieces and parts its kernels and copy threads work on.
// Pure host code (no HIP, no context), so a stand-alone program can test it:
// tests/native/hostplan_check.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rsp {

constexpr size_t kHostPiece = 8u << 20;        // pinned ring piece
constexpr size_t kHostChunkBytes = 32u << 20;  // device-side input bytes per host chunk
                                               // (c3: 8 CPIs; tools/host_probe.py)
constexpr size_t kZcPiece = 1u << 20;          // one-chunk path: device bytes per input piece
constexpr size_t kZcMaxIn = 64u << 20;         // one-chunk calls up to this much device input
constexpr size_t kZcPart = 1u << 20;           // one-chunk path: device bytes per output part
constexpr size_t kPrefaultMin = 8u << 20;      // outputs from this size on are prefaulted
constexpr int kParts = 16;                     // one-chunk output parts in flight (one event each)

// What the copy threads do to an element between the caller's array and pinned staging.
enum class Conv { kNone, kC128toC64, kF64toF32, kF32toF64, kU8toF64 };
// bytes per element on the device side and in the caller's array (kNone: any element, in bytes)
constexpr size_t conv_dev_size(Conv c) { return c == Conv::kC128toC64 ? 8 : (c == Conv::kNone || c == Conv::kU8toF64) ? 1 : 4; }
constexpr size_t conv_host_size(Conv c) { return c == Conv::kNone ? 1 : c == Conv::kC128toC64 ? 16 : 8; }
// the caller's byte offset / count of a device-side one
constexpr size_t conv_host_bytes(Conv c, size_t dev_bytes) { return dev_bytes / conv_dev_size(c) * conv_host_size(c); }

// Piece size of a DMA-ring transfer of `bytes`: the ring's 8 MiB, but at least four pieces per
// transfer down to 1 MiB, so a small call (one CPI: 8 MiB of C128 echo) still overlaps its
// memcpy with its DMA.
inline size_t piece_for(size_t bytes, size_t ring_piece = kHostPiece) {
    size_t p = (bytes / 4 + 4095) & ~(size_t)4095;
    if (p < ((size_t)1 << 20)) p = (size_t)1 << 20;
    return p < ring_piece ? p : ring_piece;
}

// Host chunks of a batch: nk chunks of K CPIs, the last one short.  host_chunk 0: by bytes.
struct HostChunks {
    int64_t batch, K, nk;
    int64_t size(int64_t k) const { return k == nk - 1 ? batch - k * K : K; }
};
inline HostChunks host_chunks(int64_t batch, int64_t host_chunk, size_t dev_cpi) {
    int64_t K = host_chunk > 0 ? host_chunk : (int64_t)(kHostChunkBytes / (dev_cpi ? dev_cpi : 1));
    if (K > batch) K = batch;
    if (K < 1) K = 1;
    return {batch, K, (batch + K - 1) / K};
}

// A call runs the one-chunk pinned path when its device input fits kZcMaxIn, every output plane
// can have a part of its own, and the contiguous (not transposed) sides are whole 4-byte words
// (launch_copy_words).
inline bool zc_eligible(size_t dbytes, int nout, int64_t batch, size_t ocells, bool in_tr, bool out_tr) {
    return dbytes <= kZcMaxIn && (int64_t)nout * batch <= kParts && (out_tr || ocells % 4 == 0) &&
           (in_tr || dbytes % 4 == 0);
}

// One-chunk input, transposed: `planes` planes of [rows][rowlen] elements of `es` device bytes;
// a piece = rows [r0, r0 + rows) of one plane, ~piece bytes in steps of 32 rows.
struct RowPiece { int64_t plane, r0, rows; };
inline std::vector<RowPiece> zc_in_rows(int64_t planes, int64_t rows, int64_t rowlen, size_t es, size_t piece) {
    int64_t rp = (int64_t)(piece / ((size_t)rowlen * es)) / 32 * 32;
    if (rp < 32) rp = 32;
    std::vector<RowPiece> v;
    for (int64_t k = 0; k < planes; ++k)
        for (int64_t r0 = 0; r0 < rows; r0 += rp) v.push_back({k, r0, r0 + rp < rows ? rp : rows - r0});
    return v;
}

// Contiguous pieces of `elems` elements: [off, off + n), `step` elements rounded up to 1024.
struct Span { size_t off, n; };
inline std::vector<Span> spans(size_t elems, size_t step) {
    step = (step + 1023) / 1024 * 1024;
    if (step < 1024) step = 1024;
    std::vector<Span> v;
    for (size_t off = 0; off < elems; off += step) v.push_back({off, elems - off < step ? elems - off : step});
    return v;
}
// One-chunk input, contiguous: ~piece bytes of `es`-byte elements each.
inline std::vector<Span> zc_in_spans(size_t elems, size_t es, size_t piece) { return spans(elems, piece / es); }

// One-chunk outputs: output k is `batch` planes of [V][Ro] cells of es[k] device bytes.  Each
// plane goes in parts of >= ~part_bytes (a part costs a kernel and an event: at c3, 2 parts of
// the 2 MiB RDM beat 4 of 512 KiB; executeCFAR's ~170 KB segments go whole), all outputs
// together within kParts whenever zc_eligible() held.  Part = cells [off, off + n) of output k
// in the caller's order; transposed (the caller's [Ro][V]), it is range bins [c0, c0 + cols) of
// plane b, in steps of 32 bins.
struct OutPart {
    int k;
    size_t off, n;
    int64_t b, c0, cols;   // transposed only
};
inline std::vector<OutPart> zc_out_parts(const size_t* es, int nout, int64_t batch, int64_t V, int64_t Ro, bool tr,
                                         size_t part_bytes) {
    const size_t cells = (size_t)V * Ro, ocells = (size_t)batch * cells;
    int64_t budget = kParts / ((int64_t)nout * batch);
    if (budget < 1) budget = 1;
    std::vector<OutPart> v;
    for (int k = 0; k < nout; ++k) {
        int64_t per_plane = (int64_t)((cells * es[k] + part_bytes / 2) / part_bytes);
        per_plane = per_plane < 1 ? 1 : (per_plane > budget ? budget : per_plane);
        if (tr) {
            int64_t cp = (Ro + per_plane - 1) / per_plane;
            cp = (cp + 31) / 32 * 32;
            for (int64_t b = 0; b < batch; ++b)
                for (int64_t c0 = 0; c0 < Ro; c0 += cp) {
                    const int64_t cols = c0 + cp < Ro ? cp : Ro - c0;
                    v.push_back({k, (size_t)(b * Ro + c0) * V, (size_t)cols * V, b, c0, cols});
                }
        } else {
            const size_t nparts = (size_t)(per_plane * batch);
            for (const Span& s : spans(ocells, (ocells + nparts - 1) / nparts)) v.push_back({k, s.off, s.n, 0, 0, 0});
        }
    }
    return v;
}

}  // namespace rsp
