// rsp_measure_math.h -- the per-hit arithmetic of the post-detection measurement
// (motionParaMeasure.m:17-86), on values: MATLAB's colon, the not-a-knot spline, its first
// maximum on the 1/interp grid, the edge re-anchoring of the cells and the three estimates.
// No HIP includes and no pointers into device memory: measure_kernel (rsp_measure.hip) and a
// host program (tests/native/measure_math_check.cpp) compile the same definitions.
// Everything is fp64 with contraction off, in the operation order of oracle/measure_ref.py, so
// the results are bit-identical to it.  A host build adds -ffp-contract=off (g++ ignores the
// clang pragma).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RSP_MM_HD __host__ __device__
#define RSP_MM_HDI __host__ __device__ __forceinline__
#else
#define RSP_MM_HD inline
#define RSP_MM_HDI inline
#endif
#if defined(__clang__)
#define RSP_MM_NO_CONTRACT _Pragma("clang fp contract(off)")
#define RSP_MM_UNROLL _Pragma("unroll")
#else
#define RSP_MM_NO_CONTRACT
#define RSP_MM_UNROLL
#endif

namespace rsp {

// motionParaMeasure.m's scalar arguments (rsp_measure_params).
struct MeasureArgs {
    int extra_dots, r_interp, v_interp, mtd0_num, beam_pos_num;
    double delta_r, delta_v, k_value, beam_angle_step, ele_comp, ele_sys_err;
    int64_t ld, cs;   // row pitch and CPI stride of the planes, in elements
};

// MATLAB's a:d:b element i of n (colon: first half from a, second half from b).
RSP_MM_HDI double colon_at(double a, double d, double b, int i, int n) {
    RSP_MM_NO_CONTRACT
    return 2 * i < n ? a + (double)i * d : b - (double)(n - 1 - i) * d;
}

// Second derivatives of the not-a-knot cubic spline through y[0..N) at unit-spaced knots
// (oracle/measure_ref.py spline_m).
template <int N>
RSP_MM_HDI void spline_m(const double (&y)[N], double (&m)[N]) {
    RSP_MM_NO_CONTRACT
    if constexpr (N == 3) {
        const double c = y[2] - 2.0 * y[1] + y[0];
        m[0] = c;
        m[1] = c;
        m[2] = c;
    } else {
        double d[N - 2];
        RSP_MM_UNROLL
        for (int i = 1; i < N - 1; ++i) d[i - 1] = 6.0 * (y[i + 1] - 2.0 * y[i] + y[i - 1]);
        m[1] = d[0] / 6.0;
        m[N - 2] = d[N - 3] / 6.0;
        constexpr int K = N - 4;
        if constexpr (K > 0) {
            double rhs[K], c[K], g[K];
            RSP_MM_UNROLL
            for (int i = 0; i < K; ++i) rhs[i] = d[i + 1];
            rhs[0] -= m[1];
            rhs[K - 1] -= m[N - 2];
            c[0] = 1.0 / 4.0;
            g[0] = rhs[0] / 4.0;
            RSP_MM_UNROLL
            for (int i = 1; i < K; ++i) {
                const double den = 4.0 - c[i - 1];
                c[i] = 1.0 / den;
                g[i] = (rhs[i] - g[i - 1]) / den;
            }
            m[2 + K - 1] = g[K - 1];
            RSP_MM_UNROLL
            for (int i = K - 2; i >= 0; --i) m[2 + i] = g[i] - c[i] * m[2 + i + 1];
        }
        m[0] = 2.0 * m[1] - m[2];
        m[N - 1] = 2.0 * m[N - 2] - m[N - 3];
    }
}

// The 1-based cell of the first maximum of the spline through y on cells first..first+N-1,
// sampled at first : 1/interp : first+N-1 (motionParaMeasure.m:36-42, :63-69).  Each interval
// j is evaluated in Horner form y_j + u*(b_j + u*(c_j + u*d_j)) (oracle/measure_ref.py
// spline_eval); the samples are walked interval by interval (their abscissae are increasing),
// so every coefficient stays in a register.
template <int N>
RSP_MM_HD double refine(const double (&y)[N], int first, int interp) {
    RSP_MM_NO_CONTRACT
    double m[N];
    spline_m<N>(y, m);
    double cb[N - 1], cc[N - 1], cd[N - 1];
    RSP_MM_UNROLL
    for (int j = 0; j < N - 1; ++j) {
        cb[j] = (y[j + 1] - y[j]) - (2.0 * m[j] + m[j + 1]) / 6.0;
        cc[j] = m[j] / 2.0;
        cd[j] = (m[j + 1] - m[j]) / 6.0;
    }
    const double a = (double)first, b = (double)(first + N - 1);
    const double d = 1.0 / (double)interp;
    const int n = (int)floor((b - a) / d + 1e-10) + 1;
    double best = -INFINITY, qbest = a;
    int i = 0;
    RSP_MM_UNROLL
    for (int j = 0; j < N - 1; ++j) {
        for (; i < n; ++i) {
            const double q = colon_at(a, d, b, i, n);
            const double t = q - a;
            int jj = (int)floor(t);
            jj = jj < 0 ? 0 : (jj > N - 2 ? N - 2 : jj);
            if (jj > j) break;
            const double u = t - (double)j;
            const double v = y[j] + u * (cb[j] + u * (cc[j] + u * cd[j]));
            if (v > best) {
                best = v;
                qbest = q;
            }
        }
    }
    return qbest;
}

// motionParaMeasure.m:22-33 / :49-60: the first of the 2e+1 cells around `center` (1-based),
// moved up to lo or down to hi by anchoring on a member of the set; false where the
// reference's find() comes back empty or the cells leave 1..size (a MATLAB error there).
RSP_MM_HDI bool fix_cells(int center, int e, int lo, int hi, int size, int* first) {
    int f = center - e;
    if (f < lo) {
        if (lo > f + 2 * e) return false;
        f = lo;
    }
    if (f + 2 * e > hi) {
        if (hi < f) return false;
        f = hi - 2 * e;
    }
    if (f < 1 || f + 2 * e > size) return false;
    *first = f;
    return true;
}

// The three estimates of the hit at 1-based cell (v1, r1) from the values around it: fr / fv the
// sum-channel values of the range cells rf..rf+N-1 of row v1 and of the velocity cells
// vf..vf+N-1 of column r1 (rf, vf from fix_cells), vs = vScale at the velocity cells, rs =
// rScale(r1), s_hit / d_hit the hit's own sum and difference amplitudes.
template <int E>
RSP_MM_HD void measure_values(const float (&fr)[2 * E + 1], const float (&fv)[2 * E + 1],
                              const double (&vs)[2 * E + 1], float s_hit, float d_hit, double rs, int r1, int rf,
                              int vf, const MeasureArgs& a, double* est) {
    RSP_MM_NO_CONTRACT
    constexpr int N = 2 * E + 1;
    double y[N];
    RSP_MM_UNROLL
    for (int k = 0; k < N; ++k) y[k] = (double)fr[k];
    const double r_max = refine<N>(y, rf, a.r_interp);
    RSP_MM_UNROLL
    for (int k = 0; k < N; ++k) y[k] = (double)fv[k];
    const double v_max = refine<N>(y, vf, a.v_interp);
    const double t = trunc(v_max);
    const int kv = (int)t - vf;   // 0..N-1: v_max lies in [vf, vf+N-1]
    double vsel = vs[0];
    RSP_MM_UNROLL
    for (int k = 1; k < N; ++k)
        if (kv == k) vsel = vs[k];
    est[0] = rs + (r_max - (double)r1) * a.delta_r;                                  // :43
    est[1] = vsel - (v_max - t) * a.delta_v;                                         // :70
    const double ratio = (double)d_hit / (double)s_hit;                              // :78
    est[2] = (double)a.beam_pos_num * a.beam_angle_step + 2.5 - ratio * a.k_value + a.ele_comp + a.ele_sys_err;   // :79
}

}  // namespace rsp
