// rsp_fuse_math.h -- the per-hit arithmetic of rsp_beam_elev_dev (include/rsp.h): the
// elevation of a fused hit from the amplitudes of its peak beam and the beam on either side.
// No HIP includes and no pointers into device memory: elev_kernel (rsp_fuse.hip) and a host program
// (tests/native/fuse_math_check.cpp) compile the same definitions.  Everything is fp64 with
// contraction off, in the operation order of include/rsp.h's rule and of tests/fuse_ref.py; a host
// build adds -ffp-contract=off (g++ ignores the clang pragma).
#pragma once
#include <math.h>
#include <stdint.h>

#include "rsp_measure_math.h"   // RSP_MM_HDI, RSP_MM_NO_CONTRACT

namespace rsp {

// k: the peak beam (0 <= k < beams); x: the beam centres; am, a0, ap: the amplitudes of beams k-1, k,
// k+1 at the cell (am / ap are not looked at where k is the first / last beam, or with law 0).
// *three = true where the result came from the three beams (clamped or not), false where it is x[k].
RSP_MM_HDI double fuse_elev(int law, int k, int beams, const double* x, float am, float a0, float ap, bool* three) {
    RSP_MM_NO_CONTRACT
    *three = false;
    const double x0 = x[k];
    if (law == 0 || k == 0 || k == beams - 1) return x0;
    const double xm = x[k - 1], xp = x[k + 1];
    const double dam = (double)am, da0 = (double)a0, dap = (double)ap;
    if (law == 1) {
        const double wm = dam * dam, w0 = da0 * da0, wp = dap * dap;
        const double num = (wm * xm + w0 * x0) + wp * xp;
        const double den = (wm + w0) + wp;
        if (den == 0.0 || !isfinite(den)) return x0;
        *three = true;
        return num / den;
    }
    if (!(dam > 0.0) || !(da0 > 0.0) || !(dap > 0.0) || !isfinite(dam) || !isfinite(da0) || !isfinite(dap)) return x0;
    const double ym = log(dam), y0 = log(da0), yp = log(dap);
    const double dm = x0 - xm, dp = x0 - xp;
    const double A = y0 - yp, B = y0 - ym;
    const double den = dm * A - dp * B;
    const double xv = x0 - 0.5 * (dm * dm * A - dp * dp * B) / den;
    if (den * (xp - xm) <= 0.0 || !isfinite(xv)) return x0;
    *three = true;
    const double lo = xm < xp ? xm : xp, hi = xm < xp ? xp : xm;
    return xv < lo ? lo : (xv > hi ? hi : xv);
}

}  // namespace rsp
