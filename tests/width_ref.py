"""fp64 restatement of MatlabProcess_xuzerui/CFAR_WangCai/ampConstrWidthEst.m in plain numpy, and
the seeded scenes the width tests share.

    widthDots = ampConstrWidthEst(specData, ampConstr, interpFlag, interpTimes)

  :3      y = abs(fftshift(specData))            (a rotation by floor(V/2), odd V included)
  :6-9    s = interp1(0:V-1, y, 0:1/interpTimes:V-1, 'spline') with interpFlag, else s = y
  :18-20  M1 = max(s); specDataScaled = 20*log10(s ./ M1)
  :37-44  the samples with specDataScaled >= ampConstr: abscissa of the last minus the first, 0 if none

interp1's 'spline' is the not-a-knot cubic spline; at unit knots its second derivatives solve
m[i-1] + 4 m[i] + m[i+1] = 6 (y[i+1] - 2 y[i] + y[i-1]) with m[0] = 2 m[1] - m[2] and its mirror
(own Thomas solve below, all columns at once; no scipy).  Each sample is evaluated as ppval does:
interval j = floor(x) (at most V-2), u = x - j, y_j + u (b_j + u (c_j + u d_j)).

log10 of a negative number is complex in MATLAB and >= compares real parts, so the test is
20*log10(|s_i| / M1) >= ampConstr: this is what `width` evaluates, with numpy's log10 on the
modulus.  0/0 is NaN and compares false: an all-zero column selects nothing, width 0.

`width` returns, per column, first / last (0-based indices on the 1/interp grid, -1 when nothing
is selected), widthDots and margin = min_i | |s_i| - 10^(a/20) M1 | / M1: how far the nearest
sample lies from the level, relative to the maximum (inf where M1 is not positive).
"""
import math

import numpy as np

TIE = 1e-9          # margin at or below this: a tie column, left out of an integer comparison
TIE_CAP = 0.01      # at most this share of a test's computed columns may be ties


def colon_unit(V, interp):
    """MATLAB's 0:1/interp:V-1 (first half from 0, second half back from V-1)."""
    d = 1.0 / interp
    n = int(math.floor((V - 1) / d + 1e-10)) + 1
    i = np.arange(n, dtype=np.float64)
    return np.where(2 * i < n, i * d, (V - 1) - (n - 1 - i) * d)


def spline_m(y):
    """Second derivatives [V][n] of the not-a-knot splines through the columns of y [V][n], V >= 4."""
    y = np.asarray(y, np.float64)
    V = y.shape[0]
    if V < 4:
        raise ValueError("spline_m: V = %d < 4" % V)
    m = np.zeros_like(y)
    d = 6.0 * (y[2:] - 2.0 * y[1:-1] + y[:-2])      # d[i-1] of row i = 1..V-2
    m[1] = d[0] / 6.0                               # row 1 with m[0] = 2 m[1] - m[2]: 6 m[1] = d
    m[V - 2] = d[V - 3] / 6.0
    K = V - 4                                       # unknowns m[2] .. m[V-3]
    if K > 0:
        rhs = d[1:V - 3].copy()
        rhs[0] -= m[1]
        rhs[-1] -= m[V - 2]
        c = np.zeros(K)
        g = np.zeros_like(rhs)
        c[0] = 0.25
        g[0] = rhs[0] / 4.0
        for i in range(1, K):
            den = 4.0 - c[i - 1]
            c[i] = 1.0 / den
            g[i] = (rhs[i] - g[i - 1]) / den
        x = np.zeros_like(rhs)
        x[-1] = g[-1]
        for i in range(K - 2, -1, -1):
            x[i] = g[i] - c[i] * x[i + 1]
        m[2:V - 2] = x
    m[0] = 2.0 * m[1] - m[2]
    m[V - 1] = 2.0 * m[V - 2] - m[V - 3]
    return m


def spline_eval(y, m, x):
    """The splines (y, m) [V][n] at the abscissae x [k]: [k][n]."""
    V = y.shape[0]
    j = np.clip(np.floor(x).astype(np.int64), 0, V - 2)
    u = (x - j)[:, None]
    b = (y[j + 1] - y[j]) - (2.0 * m[j] + m[j + 1]) / 6.0
    c = m[j] / 2.0
    d = (m[j + 1] - m[j]) / 6.0
    return y[j] + u * (b + u * (c + u * d))


def samples(amp, interp, interp_flag=True, shift=True):
    """(x, s): the abscissae [k] and the samples [k][n] of the columns of amp [V][n] (magnitudes)."""
    y = np.asarray(amp, np.float64)
    if y.ndim == 1:
        y = y[:, None]
    V = y.shape[0]
    if shift:
        y = np.roll(y, V // 2, axis=0)              # fftshift along the column
    if not interp_flag:
        return np.arange(V, dtype=np.float64), y
    x = colon_unit(V, interp)
    if interp == 1:
        return x, y                                 # a spline sampled at its own knots
    return x, spline_eval(y, spline_m(y), x)


def select(x, s, amp_constr, interp):
    """:18-44 on samples s [k][n] -> (first, last, widthDots, margin), each [n]."""
    n = s.shape[1]
    first = np.full(n, -1, np.int64)
    last = np.full(n, -1, np.int64)
    width = np.zeros(n)
    margin = np.full(n, np.inf)
    M1 = s.max(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        scaled = 20.0 * np.log10(np.abs(s / M1[None, :]))
        sel = scaled >= amp_constr                  # NaN compares false
    lvl = 10.0 ** (amp_constr / 20.0)
    for c in range(n):
        idx = np.flatnonzero(sel[:, c])
        if idx.size:
            first[c], last[c] = idx[0], idx[-1]
            width[c] = abs(x[idx[-1]] - x[idx[0]])
        if M1[c] > 0:
            margin[c] = np.min(np.abs(np.abs(s[:, c]) - lvl * M1[c])) / M1[c]
    return first, last, width, margin


def width(spec, amp_constr, interp_flag, interp, shift=True):
    """ampConstrWidthEst over the columns of spec [V] or [V][n] (complex or real; abs is taken
    here) -> (first, last, widthDots, margin), each [n].  first / last index the 1/interp grid
    (the knot grid without interp_flag)."""
    a = np.abs(np.asarray(spec))
    x, s = samples(a, interp, interp_flag, shift)
    return select(x, s, amp_constr, interp if interp_flag else 1)


# ------------------------------------------------------------------ the seeded scenes
INTERPS = (1, 3, 4, 8, 64)
LEVELS = (-3.0, -6.0, -20.0, -40.0)
SHAPES = ((4, 17), (5, 24), (33, 17), (128, 24), (332, 17), (2048, 24))     # (V, R), ld = R


def interps_for(V):
    return tuple(i for i in INTERPS if i < 64 or V <= 128)


def scene(V, n, seed):
    """float32 [V][n]: Rayleigh noise (sigma 1) plus two lines of different strength per column
    (a few bins wide, circular in V); every second column has a zeroed band at both ends of V."""
    rng = np.random.default_rng(seed)
    a = rng.rayleigh(1.0, size=(V, n))
    v = np.arange(V)[:, None]
    for lo, hi in ((40.0, 120.0), (8.0, 30.0)):
        v0 = rng.uniform(0, V, size=n)[None, :]
        amp = rng.uniform(lo, hi, size=n)[None, :]
        sig = rng.uniform(0.7, 2.5, size=n)[None, :]
        dv = (v - v0 + V / 2.0) % V - V / 2.0
        a = a + amp * np.exp(-0.5 * (dv / sig) ** 2)
    nz = min(7, V // 8)
    if nz:
        a[:nz, 1::2] = 0.0
        a[V - nz + 1:, 1::2] = 0.0
    return a.astype(np.float32)


def sparse_flags(V, n, hits, seed):
    """uint8 [V][n] with about `hits` ones."""
    rng = np.random.default_rng(seed)
    f = np.zeros((V, n), np.uint8)
    f[rng.integers(0, V, size=hits), rng.integers(0, n, size=hits)] = 1
    return f


def edge_flags(V, n, group=16):
    """uint8 [V][n]: one hit in each of the window's edge columns and in the columns either side
    of every column-group boundary a kernel may have (16 and 64), in different rows."""
    f = np.zeros((V, n), np.uint8)
    cols = {0, n - 1}
    for g in (group, 64):
        for b in range(g, n, g):
            cols.update((b - 1, b))
    for k, c in enumerate(sorted(cols)):
        f[(7 * k + 3) % V, c] = 1
    return f, sorted(cols)


# the window case: 96 x 130 at column 7 of ld = 160 planes, CPI stride padded by 53 elements
WIN = dict(V=96, R=130, col0=7, ld=160, cs=96 * 160 + 53, batch=3)
# the DMX case: one 2048 x 574 CPI as its short and long windows
DMX = dict(V=2048, Rp=574, windows=((0, 62), (62, 574)), hits=1044)


def compare(span, count, amp, need, amp_constr, interp, shift):
    """Check one CPI's spans [R][2] and count against the restatement on amp [V][R]; need: bool [R],
    the columns that must be computed.  Returns (tested, ties); raises AssertionError on a
    difference outside ties, a wrong count, or a computed mark on a column that must not be."""
    span = np.asarray(span)
    R = amp.shape[1]
    assert span.shape == (R, 2)
    assert int(count) == int(need.sum()), "count %d, %d columns carry a hit" % (int(count), int(need.sum()))
    assert (span[~need] == -1).all(), "a column without a hit is not {-1, -1}"
    idx = np.flatnonzero(need)
    if idx.size == 0:
        return 0, 0
    first, last, _, margin = width(amp[:, idx], amp_constr, True, interp, shift)
    tie = margin <= TIE
    ok = ~tie
    got = span[idx]
    bad = ok & ((got[:, 0] != first) | (got[:, 1] != last))
    assert not bad.any(), "columns %s: got %s, want %s (margins %s)" % (
        idx[bad][:8].tolist(), got[bad][:8].tolist(), np.stack([first, last], 1)[bad][:8].tolist(),
        margin[bad][:8].tolist())
    return int(idx.size), int(tie.sum())
