"""fp64 restatement of MatlabProcess_xuzerui/fun_SCR.m and fun_add_clutter.m (the target
injection of main.m:183-194), written from their semantics, for both power modes:

    P_s = mean(Echo_simu(1, points).^2) + eps                 row 1, before any scaling
    for every row i:  P_echo = mean(echo(i, points).^2)
                      g = P_echo * 10^((SCR + off)/10) / P_s
                      Echo_simu(i, points) = Echo_simu(i, points) * sqrt(g)
    out(i, :) = Echo_simu(i, :) + echo(i, 1:point_prt)

AS_WRITTEN: `.^2` of complex data is the complex square, g is complex and sqrt the principal
root.  MATLAB stores a value whose imaginary part is zero as real, so the root of a negative
real g is +j sqrt|g| (numpy would follow the sign of a -0 imaginary part).  ABS2: mean(|x|^2),
g real.  echo_simu() is the materialised Echo_simu of a point-target plan: per segment the
waveform at a delay column, truncated at the segment's end, times exp(j dphi m) at pulse m.
"""
import numpy as np

ABS2, AS_WRITTEN = 0, 1
EPS = 2.0 ** -52
LEGACY_SEGMENTS = ((0, 82), (82, 242), (324, 707))
LEGACY_SEG_DB = (10.0, 0.0, 0.0)


def power_sum(x, power):
    """sum(x.^2) (complex) or sum(|x|^2) over a vector, complex128."""
    x = np.asarray(x, np.complex128)
    return complex(np.sum(x * x)) if power == AS_WRITTEN else complex(float(np.sum(x.real ** 2 + x.imag ** 2)), 0.0)


def _sqrt(g):
    g = complex(g)
    if g.imag == 0.0:                      # stored as real: sqrt of a negative real is +j sqrt|g|
        return complex(np.sqrt(g.real), 0.0) if g.real >= 0 else complex(0.0, np.sqrt(-g.real))
    return complex(np.sqrt(np.complex128(g)))


def gain_from_sums(power, sum_simu, sum_clutter, n, scr_db):
    """sqrt(g) from the two sums over a segment of n columns."""
    sum_simu, sum_clutter = complex(sum_simu), complex(sum_clutter)
    if power == ABS2:
        sum_simu, sum_clutter = complex(sum_simu.real, 0.0), complex(sum_clutter.real, 0.0)
    P_s = sum_simu / n + EPS
    P_echo = sum_clutter / n
    with np.errstate(all="ignore"):
        g = np.complex128(P_echo * 10.0 ** (scr_db / 10.0)) / np.complex128(P_s)
    return _sqrt(g)


def gains(simu, clutter, scr_db, segments, seg_db, power):
    """complex128 [P][nseg]: sqrt(g) of every (row, segment) of one CPI, and arg(g)."""
    P = simu.shape[0]
    out = np.zeros((P, len(segments)), np.complex128)
    for s, (a, n) in enumerate(segments):
        ss = power_sum(simu[0, a:a + n], power)
        for i in range(P):
            out[i, s] = gain_from_sums(power, ss, power_sum(clutter[i, a:a + n], power), n, scr_db + seg_db[s])
    return out


def fun_SCR(Echo_simu, echo, SCR, segments=LEGACY_SEGMENTS, seg_db=LEGACY_SEG_DB, power=AS_WRITTEN):  # noqa: N802,N803
    """One CPI, P x R; the echo may be wider.  Returns (Echo_simu_STC complex128, gains [P][nseg])."""
    x = np.array(Echo_simu, np.complex128)
    e = np.asarray(echo, np.complex128)
    g = gains(x, e, float(SCR), segments, seg_db, power)
    for s, (a, n) in enumerate(segments):
        x[:, a:a + n] *= g[:, s:s + 1]
    return x, g


def fun_add_clutter(Echo_simu_STC, echo):  # noqa: N802,N803
    x = np.asarray(Echo_simu_STC, np.complex128)
    return x + np.asarray(echo, np.complex128)[:x.shape[0], :x.shape[1]]


def inject(simu, clutter, scr_db, segments, seg_db=None, power=ABS2, add_clutter=True):
    """The batched form: simu [B][P][R], clutter [K][P][>=R] (CPI b uses b % K), scr_db [B] or a
    scalar.  Returns (out complex128 [B][P][R], gains [B][P][nseg])."""
    simu = np.asarray(simu)
    clutter = np.asarray(clutter)
    B = simu.shape[0]
    seg_db = [0.0] * len(segments) if seg_db is None else seg_db
    scr = np.broadcast_to(np.asarray(scr_db, np.float64), (B,))
    out = np.empty(simu.shape, np.complex128)
    gs = np.empty((B, simu.shape[1], len(segments)), np.complex128)
    for b in range(B):
        c = clutter[b % clutter.shape[0]]
        y, gs[b] = fun_SCR(simu[b], c, scr[b], segments, seg_db, power)
        out[b] = fun_add_clutter(y, c) if add_clutter else y
    return out, gs


def arg_margin(gs):
    """pi - max|arg g| over the gains sqrt(g) of inject(): how far every g stays from the
    negative real axis, where the principal root flips sign."""
    g2 = gs[gs != 0] ** 2
    return float(np.pi - np.max(np.abs(np.angle(g2)))) if g2.size else float(np.pi)


def echo_simu(P, R, segments, waveforms, delay, dphi):
    """Materialised Echo_simu of a point-target plan, complex128 [B][P][R]: segment s = (start,
    length) holds waveforms[s] from column start + delay[b][s] (delay < 0 or >= length: no
    target), cut at the segment's end, times exp(j dphi[b] m) at pulse m = 0..P-1."""
    delay = np.asarray(delay)
    B = delay.shape[0]
    x = np.zeros((B, P, R), np.complex128)
    m = np.arange(P)
    for b in range(B):
        dop = np.exp(1j * float(dphi[b]) * m)
        for s, (a, n) in enumerate(segments):
            d = int(delay[b, s])
            if d < 0 or d >= n:
                continue
            w = np.asarray(waveforms[s], np.complex128)[:n - d]
            x[b, :, a + d:a + d + len(w)] += np.outer(dop, w)
    return x
