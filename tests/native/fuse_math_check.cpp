// Stand-alone run of rsp_fuse_math.h on the host (tests/test_fuse_cpu.py): the definition elev_kernel
// compiles, fed from a file, its results written as raw bits for the test to compare with
// tests/fuse_ref.py.  Built with -ffp-contract=off, once plain and once with the address and
// undefined-behaviour sanitizers.
//   fuse_math_check IN OUT   IN:  records {int32 law, k, beams, 0; double x[32]; float am, a0, ap, 0}
//                            OUT: {uint64 bits of fuse_elev()'s result; int32 three, 0} per record
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "rsp_fuse_math.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 64;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = in ? std::fopen(argv[2], "wb") : nullptr;
    if (!in || !out) {
        std::fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
        if (in) std::fclose(in);
        return 66;
    }
    int rc = 0;
    for (;;) {
        int32_t h[4];
        double x[32];
        float a[4];
        const size_t got = std::fread(h, sizeof(int32_t), 4, in);
        if (got == 0) break;
        if (got != 4 || std::fread(x, sizeof(double), 32, in) != 32 || std::fread(a, sizeof(float), 4, in) != 4 ||
            h[0] < 0 || h[0] > 2 || h[2] < 2 || h[2] > 32 || h[1] < 0 || h[1] >= h[2]) {
            rc = 2;
            break;
        }
        bool three = false;
        const double e = rsp::fuse_elev(h[0], h[1], h[2], x, a[0], a[1], a[2], &three);
        uint64_t u;
        std::memcpy(&u, &e, sizeof u);
        const int32_t t[2] = {three ? 1 : 0, 0};
        if (std::fwrite(&u, sizeof u, 1, out) != 1 || std::fwrite(t, sizeof(int32_t), 2, out) != 2) {
            rc = 3;
            break;
        }
    }
    std::fclose(in);
    if (std::fclose(out) != 0 && rc == 0) rc = 3;
    if (rc) std::fprintf(stderr, "fuse_math_check: failed (%d)\n", rc);
    return rc;
}
