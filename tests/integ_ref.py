"""Restatement of rsp_integrate_dev / rsp_binint_dev (include/rsp.h: post-detection integration over the
CPIs of a dwell), for the tests: numpy, one CPI at a time in batch order, every fp32 addition a separate
float32 add in the stated order, the ring and meta exactly as specified.

    run(x, n, hist, meta, shift=None, slot=None, m=None, spread=0) -> (out, neff)

x is [batch][V][R] float32 (sum form, m None) or uint8 (binary form, m = 1..n); hist [slots][n-1][V][R]
of x's dtype and meta int32 [slots][2] are updated in place.  Written for clarity, not speed.
"""
import numpy as np


def shifted(plane, sh):
    """term[v][r] = plane[v][r - sh[v]], zero (+0.0 / no hit) where the source column is outside [0, R).
    Nothing wraps; any integer shift is legal."""
    V, R = plane.shape
    out = np.zeros_like(plane)
    r = np.arange(R, dtype=np.int64)
    for v in range(V):
        c = r - int(sh[v])
        ok = (c >= 0) & (c < R)
        out[v, ok] = plane[v, c[ok]]
    return out


def spread_term(hit, sh, spread):
    """bool [V][R]: any of the columns r - sh[v] - spread .. r - sh[v] + spread that lie inside the window
    is set in hit[v]."""
    V, R = hit.shape
    out = np.zeros((V, R), bool)
    r = np.arange(R, dtype=np.int64)
    for v in range(V):
        for d in range(-int(spread), int(spread) + 1):
            c = r - int(sh[v]) + d
            ok = (c >= 0) & (c < R)
            out[v, ok] |= hit[v, c[ok]]
    return out


def step(x0, past, n, shift, m=None, spread=0):
    """One CPI: x0 [V][R] and past = [x_1, x_2, ..] (the planes 1, 2, .. CPIs back, at most n-1)."""
    V, R = x0.shape
    if m is None:
        acc = x0.astype(np.float32).copy()
        with np.errstate(invalid="ignore", over="ignore"):
            for i, xi in enumerate(past, 1):
                sh = np.zeros(V, np.int64) if shift is None else shift[i - 1]
                acc = (acc + shifted(xi, sh)).astype(np.float32)   # the out-of-window term is +0.0f, added
        return acc
    cnt = (x0 != 0).astype(np.int32)
    for i, xi in enumerate(past, 1):
        sh = np.zeros(V, np.int64) if shift is None else shift[i - 1]
        cnt += spread_term(xi != 0, sh, spread).astype(np.int32)
    return (cnt >= int(m)).astype(np.uint8)


def run(x, n, hist, meta, shift=None, slot=None, m=None, spread=0):
    x = np.asarray(x)
    B = x.shape[0]
    slots = meta.shape[0]
    out = np.empty_like(x)
    neff = np.empty(B, np.int32)
    for b in range(B):
        s = 0 if slot is None else int(slot[b])
        if s < 0 or s >= slots:
            neff[b] = 1
            out[b] = step(x[b], [], n, shift, m, spread)
            continue
        k = max(int(meta[s, 0]), 0)
        ne = min(n, k + 1)
        past = [hist[s, (k - i) % (n - 1)] for i in range(1, ne)]
        out[b] = step(x[b], past, n, shift, m, spread)
        neff[b] = ne
        if n > 1:
            hist[s, k % (n - 1)] = x[b]
        meta[s, 0] = k + 1
    return out, neff


def new_state(slots, n, V, R, dtype, junk=None):
    """(hist, meta) of a reset integrator; junk: a seed that fills the ring with arbitrary bytes
    instead of zeros (a reset does not clear it)."""
    shape = (slots, max(n - 1, 0), V, R)
    if junk is None:
        hist = np.zeros(shape, dtype)
    else:
        rng = np.random.default_rng(junk)
        hist = rng.integers(0, 256, size=int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=np.uint8) \
            .view(dtype).reshape(shape).copy()
    return hist, np.zeros((slots, 2), np.int32)


def split_run(x, n, hist, meta, cuts, shift=None, slot=None, m=None, spread=0):
    """run() over the consecutive pieces x[cuts[i]:cuts[i+1]]; the concatenated outputs."""
    outs, neffs = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        o, ne = run(x[a:b], n, hist, meta, shift, None if slot is None else slot[a:b], m, spread)
        outs.append(o)
        neffs.append(ne)
    return np.concatenate(outs), np.concatenate(neffs)
