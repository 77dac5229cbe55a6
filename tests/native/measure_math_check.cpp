// Stand-alone run of rsp_measure_math.h on the host (tests/test_measure_cpu.py): the definitions
// measure_kernel compiles, fed from a file, their results written as raw bits for the test to
// compare with oracle/measure_ref.py.  Built with -ffp-contract=off.
//   measure_math_check refine IN OUT   IN: records {int32 e, first, interp, 0; double y[2e+1]}
//                                      OUT: one uint64 per record, the bits of refine()'s result
//   measure_math_check fix IN OUT      IN: records {int32 center, e, lo, hi, size}
//                                      OUT: {int32 ok, first} per record (first = 0 where refused)
//   measure_math_check hit IN OUT      IN: records {int32 e, r1, rf, vf, r_interp, v_interp, beam_pos_num, 0;
//                                          double delta_r, delta_v, k_value, beam_angle_step, ele_comp,
//                                          ele_sys_err, rs, vs[2e+1]; float fr[2e+1], fv[2e+1], s_hit, d_hit}
//                                      OUT: three uint64 per record, the bits of measure_values()'s estimates
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "rsp_measure_math.h"

template <int E>
static uint64_t refine_bits(const double* y, int first, int interp) {
    constexpr int N = 2 * E + 1;
    double a[N];
    for (int k = 0; k < N; ++k) a[k] = y[k];
    const double q = rsp::refine<N>(a, first, interp);
    uint64_t u;
    std::memcpy(&u, &q, sizeof u);
    return u;
}

static int run_refine(std::FILE* in, std::FILE* out) {
    for (;;) {
        int32_t h[4];
        const size_t got = std::fread(h, sizeof(int32_t), 4, in);
        if (got == 0) return 0;
        if (got != 4 || h[0] < 1 || h[0] > 4 || h[2] < 1 || h[2] > 64) return 2;
        double y[9];
        const size_t n = 2 * (size_t)h[0] + 1;
        if (std::fread(y, sizeof(double), n, in) != n) return 2;
        uint64_t u = 0;
        switch (h[0]) {
            case 1: u = refine_bits<1>(y, h[1], h[2]); break;
            case 2: u = refine_bits<2>(y, h[1], h[2]); break;
            case 3: u = refine_bits<3>(y, h[1], h[2]); break;
            default: u = refine_bits<4>(y, h[1], h[2]); break;
        }
        if (std::fwrite(&u, sizeof u, 1, out) != 1) return 3;
    }
}

static int run_fix(std::FILE* in, std::FILE* out) {
    for (;;) {
        int32_t h[5];
        const size_t got = std::fread(h, sizeof(int32_t), 5, in);
        if (got == 0) return 0;
        if (got != 5) return 2;
        int first = 0;
        const bool ok = rsp::fix_cells(h[0], h[1], h[2], h[3], h[4], &first);
        const int32_t r[2] = {ok ? 1 : 0, ok ? first : 0};
        if (std::fwrite(r, sizeof(int32_t), 2, out) != 2) return 3;
    }
}

template <int E>
static void hit_bits(const rsp::MeasureArgs& a, const int32_t* h, double rs, const double* vs, const float* f,
                     uint64_t* out) {
    constexpr int N = 2 * E + 1;
    float fr[N], fv[N];
    double v[N], est[3];
    for (int k = 0; k < N; ++k) {
        fr[k] = f[k];
        fv[k] = f[N + k];
        v[k] = vs[k];
    }
    rsp::measure_values<E>(fr, fv, v, f[2 * N], f[2 * N + 1], rs, h[1], h[2], h[3], a, est);
    std::memcpy(out, est, sizeof est);
}

static int run_hit(std::FILE* in, std::FILE* out) {
    for (;;) {
        int32_t h[8];
        const size_t got = std::fread(h, sizeof(int32_t), 8, in);
        if (got == 0) return 0;
        if (got != 8 || h[0] < 1 || h[0] > 4 || h[4] < 1 || h[4] > 64 || h[5] < 1 || h[5] > 64) return 2;
        const size_t n = 2 * (size_t)h[0] + 1;
        double d[7 + 9];
        float f[2 * 9 + 2];
        if (std::fread(d, sizeof(double), 7 + n, in) != 7 + n) return 2;
        if (std::fread(f, sizeof(float), 2 * n + 2, in) != 2 * n + 2) return 2;
        rsp::MeasureArgs a{};
        a.extra_dots = h[0];
        a.r_interp = h[4];
        a.v_interp = h[5];
        a.beam_pos_num = h[6];
        a.delta_r = d[0];
        a.delta_v = d[1];
        a.k_value = d[2];
        a.beam_angle_step = d[3];
        a.ele_comp = d[4];
        a.ele_sys_err = d[5];
        uint64_t u[3];
        switch (h[0]) {
            case 1: hit_bits<1>(a, h, d[6], d + 7, f, u); break;
            case 2: hit_bits<2>(a, h, d[6], d + 7, f, u); break;
            case 3: hit_bits<3>(a, h, d[6], d + 7, f, u); break;
            default: hit_bits<4>(a, h, d[6], d + 7, f, u); break;
        }
        if (std::fwrite(u, sizeof(uint64_t), 3, out) != 3) return 3;
    }
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s refine|fix|hit IN OUT\n", argv[0]);
        return 64;
    }
    std::FILE* in = std::fopen(argv[2], "rb");
    std::FILE* out = in ? std::fopen(argv[3], "wb") : nullptr;
    if (!in || !out) {
        std::fprintf(stderr, "cannot open %s / %s\n", argv[2], argv[3]);
        if (in) std::fclose(in);
        return 66;
    }
    int rc = 64;
    if (!std::strcmp(argv[1], "refine")) rc = run_refine(in, out);
    if (!std::strcmp(argv[1], "fix")) rc = run_fix(in, out);
    if (!std::strcmp(argv[1], "hit")) rc = run_hit(in, out);
    std::fclose(in);
    if (std::fclose(out) != 0 && rc == 0) rc = 3;
    if (rc) std::fprintf(stderr, "%s: failed (%d)\n", argv[1], rc);
    return rc;
}
