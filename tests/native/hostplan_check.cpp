// Stand-alone check of the host-buffer entry points' planning arithmetic
// (radar-signal-process_amd/csrc/rsp_hostplan.h): the one-chunk input pieces and output parts
// deliver every element exactly once, never cross a plane, keep the alignments their kernels
// need and stay within the kParts events; the ring pieces tile a transfer; the host chunks tile
// a batch.  The default plans of three known calls are pinned.
// Built and run by tests/test_hostplan_cpu.py (also with -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>

#include "rsp_hostplan.h"

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            if (++fails <= 20) std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                               \
    } while (0)

static const int64_t kDims[] = {1, 31, 32, 33, 64, 100, 1000, 1024, 1200, 4000, 4096, 16384};
static const size_t kElem[] = {1, 4, 8};
static const size_t kSizes[] = {(size_t)64 << 10, (size_t)1 << 20, (size_t)4 << 20};

// in order, disjoint, exactly [0, elems); one plane, whole rows, r0 % 32 == 0
static void check_in_rows(int64_t planes, int64_t rows, int64_t cols, size_t es, size_t piece) {
    const std::vector<rsp::RowPiece> v = rsp::zc_in_rows(planes, rows, cols, es, piece);
    size_t at = 0;   // next element expected
    for (const rsp::RowPiece& p : v) {
        CHECK(p.plane >= 0 && p.plane < planes && p.rows >= 1 && p.r0 >= 0 && p.r0 + p.rows <= rows);
        CHECK(p.r0 % 32 == 0);
        CHECK((size_t)(p.plane * rows + p.r0) * cols == at);
        at += (size_t)p.rows * cols;
    }
    CHECK(at == (size_t)planes * rows * cols);
}

// in order, disjoint, exactly [0, elems); offsets at multiples of 1024; whole words when the total is
static void check_in_spans(size_t elems, size_t es, size_t piece) {
    size_t at = 0;
    for (const rsp::Span& s : rsp::zc_in_spans(elems, es, piece)) {
        CHECK(s.off == at && s.n >= 1 && s.off % 1024 == 0);
        if (elems * es % 4 == 0) CHECK(s.n * es % 4 == 0);
        at += s.n;
    }
    CHECK(at == elems);
}

static void check_out(const size_t* es, int nout, int64_t batch, int64_t V, int64_t Ro, bool tr, size_t part) {
    const size_t cells = (size_t)V * Ro, ocells = (size_t)batch * cells;
    const std::vector<rsp::OutPart> v = rsp::zc_out_parts(es, nout, batch, V, Ro, tr, part);
    if (rsp::zc_eligible(0, nout, batch, ocells, true, tr)) CHECK(v.size() <= (size_t)rsp::kParts);
    size_t at[3] = {};   // per output: next cell expected
    int k_prev = 0;
    for (const rsp::OutPart& p : v) {
        CHECK(p.k >= k_prev && p.k < nout);
        if (p.k < 0 || p.k >= nout) return;
        k_prev = p.k;
        CHECK(p.off == at[p.k] && p.n >= 1);
        at[p.k] += p.n;
        if (tr) {
            CHECK(p.c0 % 32 == 0 && p.b >= 0 && p.b < batch && p.c0 >= 0 && p.cols >= 1 && p.c0 + p.cols <= Ro);
            CHECK(p.off == (size_t)(p.b * Ro + p.c0) * V && p.n == (size_t)p.cols * V);
        } else {
            CHECK(p.off % 1024 == 0);
            if (ocells % 4 == 0) CHECK(p.n * es[p.k] % 4 == 0);
        }
    }
    for (int k = 0; k < nout; ++k) CHECK(at[k] == ocells);
}

static void sweep() {
    for (int64_t planes = 1; planes <= 6; ++planes)
        for (int64_t rows : kDims)
            for (int64_t cols : kDims)
                for (size_t es : kElem)
                    for (size_t piece : kSizes) {
                        check_in_rows(planes, rows, cols, es, piece);
                        check_in_spans((size_t)planes * rows * cols, es, piece);
                    }
    for (int64_t batch = 1; batch <= 16; ++batch)
        for (int64_t V : kDims)
            for (int64_t Ro : kDims)
                for (int nout = 1; nout <= 3; ++nout)
                    for (int e0 = 0; e0 < 3; ++e0)
                        for (size_t part : kSizes) {
                            const size_t es[3] = {kElem[e0], kElem[(e0 + 1) % 3], kElem[(e0 + 2) % 3]};
                            check_out(es, nout, batch, V, Ro, true, part);
                            check_out(es, nout, batch, V, Ro, false, part);
                        }
    // ring pieces: within [1 MiB, kHostPiece], page multiples (so any element size divides a
    // piece's offset), tiling the transfer
    for (size_t bytes : {(size_t)1, (size_t)4096, (size_t)1 << 20, ((size_t)1 << 20) + 1, (size_t)4000 * 512 * 4,
                         (size_t)8 << 20, ((size_t)8 << 20) + 8, (size_t)31 << 20, (size_t)32 << 20, (size_t)33 << 20,
                         (size_t)1 << 30, ((size_t)5 << 30) + 12}) {
        const size_t p = rsp::piece_for(bytes);
        CHECK(p >= ((size_t)1 << 20) && p <= rsp::kHostPiece && p % 4096 == 0);
        size_t sum = 0, n = 0;
        for (size_t off = 0; off < bytes; off += p, ++n) sum += bytes - off < p ? bytes - off : p;
        CHECK(sum == bytes && n == (bytes + p - 1) / p);
        if (bytes >= ((size_t)4 << 20) && bytes <= 4 * rsp::kHostPiece) CHECK(n == 4);
    }
    // host chunks: sizes sum to the batch, only the last one short
    for (int64_t batch = 1; batch <= 40; ++batch)
        for (int64_t hc = 0; hc <= 9; ++hc)
            for (size_t cpi : {(size_t)1, (size_t)64 * 1024 * 8, (size_t)128 * 4096 * 8, (size_t)5 << 20, (size_t)32 << 20,
                               (size_t)100 << 20}) {
                const rsp::HostChunks c = rsp::host_chunks(batch, hc, cpi);
                CHECK(c.K >= 1 && c.K <= batch && c.nk >= 1);
                if (hc > 0) CHECK(c.K == (hc < batch ? hc : batch));
                else CHECK(c.K == batch || (size_t)c.K * cpi <= rsp::kHostChunkBytes || c.K == 1);
                int64_t sum = 0;
                for (int64_t k = 0; k < c.nk; ++k) {
                    const int64_t n = c.size(k);
                    CHECK(n >= 1 && n <= c.K);
                    if (k + 1 < c.nk) CHECK(n == c.K);
                    sum += n;
                }
                CHECK(sum == batch);
            }
}

// the default plans of known calls, from the formulae these functions replaced
static void pinned() {
    CHECK(rsp::kHostPiece == (size_t)8 << 20 && rsp::kHostChunkBytes == (size_t)32 << 20 && rsp::kParts == 16);
    CHECK(rsp::kZcPiece == (size_t)1 << 20 && rsp::kZcPart == (size_t)1 << 20 && rsp::kZcMaxIn == (size_t)64 << 20);
    CHECK(rsp::kPrefaultMin == (size_t)8 << 20);
    {   // one c3 CPI: C128 column-major 128 x 4096, 8 bytes per element on the device
        const std::vector<rsp::RowPiece> in = rsp::zc_in_rows(1, 4096, 128, 8, rsp::kZcPiece);
        CHECK(in.size() == 4);
        for (size_t i = 0; i < in.size(); ++i) CHECK(in[i].plane == 0 && in[i].r0 == (int64_t)i * 1024 && in[i].rows == 1024);
        const size_t es[3] = {4, 1, 1};   // RDM, flag, flagV
        CHECK(rsp::zc_eligible((size_t)128 * 4096 * 8, 3, 1, (size_t)128 * 4096, true, true));
        for (bool tr : {true, false}) {
            const std::vector<rsp::OutPart> out = rsp::zc_out_parts(es, 3, 1, 128, 4096, tr, rsp::kZcPart);
            CHECK(out.size() == 4);
            if (out.size() != 4) continue;
            CHECK(out[0].k == 0 && out[1].k == 0 && out[2].k == 1 && out[3].k == 2);
            CHECK(out[0].n == (size_t)262144 && out[1].off == (size_t)262144 && out[1].n == (size_t)262144);
            CHECK(out[2].off == 0 && out[2].n == (size_t)524288 && out[3].off == 0 && out[3].n == (size_t)524288);
            if (tr) CHECK(out[0].cols == 2048 && out[1].c0 == 2048 && out[1].cols == 2048 && out[2].cols == 4096);
        }
        const rsp::HostChunks c = rsp::host_chunks(32, 0, (size_t)128 * 4096 * 8);
        CHECK(c.K == 8 && c.nk == 4);
        CHECK(rsp::piece_for((size_t)128 * 4096 * 8) == (size_t)1 << 20);
    }
    {   // rsp_cfar_f64, V = 512, R = 4000, batch 2, column-major, with flagV
        const std::vector<rsp::RowPiece> in = rsp::zc_in_rows(2, 4000, 512, 4, rsp::kZcPiece);
        CHECK(in.size() == 16);
        for (size_t i = 0; i < in.size() && in.size() == 16; ++i)
            CHECK(in[i].plane == (int64_t)(i / 8) && in[i].r0 == (int64_t)(i % 8) * 512 && in[i].rows == (i % 8 == 7 ? 416 : 512));
        const size_t es[2] = {1, 1};
        CHECK(rsp::zc_eligible((size_t)2 * 512 * 4000 * 4, 2, 2, (size_t)2 * 512 * 4000, true, true));
        const std::vector<rsp::OutPart> out = rsp::zc_out_parts(es, 2, 2, 512, 4000, true, rsp::kZcPart);
        CHECK(out.size() == 8);
        for (size_t i = 0; i < out.size() && out.size() == 8; ++i) {
            CHECK(out[i].k == (int)(i / 4) && out[i].b == (int64_t)(i / 2 % 2));
            CHECK(out[i].c0 == (i % 2 ? 2016 : 0) && out[i].cols == (i % 2 ? 1984 : 2016));
        }
        // row-major: 1 MiB pieces of floats; each flag array in 4 parts
        CHECK(rsp::zc_in_spans((size_t)2 * 512 * 4000, 4, rsp::kZcPiece).size() == 16);
        CHECK(rsp::zc_out_parts(es, 2, 2, 512, 4000, false, rsp::kZcPart).size() == 8);
    }
    // batch 20 with flagV (64 x 1024): more than kParts planes, the DMA pipeline's
    CHECK(!rsp::zc_eligible((size_t)20 * 64 * 1024 * 4, 2, 20, (size_t)20 * 64 * 1024, true, true));
    CHECK(!rsp::zc_eligible((size_t)20 * 64 * 1024 * 4, 2, 20, (size_t)20 * 64 * 1024, false, false));
    CHECK(rsp::zc_eligible((size_t)16 * 64 * 1024 * 4, 1, 16, (size_t)16 * 64 * 1024, false, false));
    CHECK(!rsp::zc_eligible(rsp::kZcMaxIn + 4, 1, 1, 1024, true, true));
    CHECK(!rsp::zc_eligible(1024, 1, 1, 1023, true, false) && rsp::zc_eligible(1024, 1, 1, 1023, true, true));
    CHECK(!rsp::zc_eligible(1022, 1, 1, 1024, false, true) && rsp::zc_eligible(1022, 1, 1, 1024, true, true));
    // the conversions' host side of a device-side byte count
    CHECK(rsp::conv_host_bytes(rsp::Conv::kNone, 12) == 12 && rsp::conv_host_bytes(rsp::Conv::kC128toC64, 16) == 32);
    CHECK(rsp::conv_host_bytes(rsp::Conv::kF64toF32, 8) == 16 && rsp::conv_host_bytes(rsp::Conv::kF32toF64, 8) == 16);
    CHECK(rsp::conv_host_bytes(rsp::Conv::kU8toF64, 3) == 24);
}

int main() {
    sweep();
    pinned();
    if (fails) {
        std::fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    std::puts("ok");
    return 0;
}
