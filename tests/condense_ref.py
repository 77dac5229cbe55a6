"""Plain integer / fp64 restatement of plot condensation (include/rsp.h, rsp_condense_dev): the
checker of tests/test_condense_cpu.py and tests/test_gpu_condense.py.

Hits in MATLAB's find() order, components by brute-force pairwise adjacency and a breadth-first
closure, peaks by first maximum, plots sorted by the peak's find() key r*V + v.  Nothing here is
shared with the kernels.
"""
from collections import deque

import numpy as np


def hits(flag):
    """(v, r) of the nonzero cells of a V x R plane in find() order (column, then row)."""
    r, v = np.nonzero(np.asarray(flag).T)
    return v.astype(np.int64), r.astype(np.int64)


def adjacency(v, r, V, gap, wrap_v):
    """n x n boolean matrix of the definition: dv <= gap_v and dr <= gap_r."""
    dv = np.abs(v[:, None] - v[None, :])
    if wrap_v:
        dv = np.minimum(dv, V - dv)
    dr = np.abs(r[:, None] - r[None, :])
    return (dv <= gap[0]) & (dr <= gap[1])


def components(v, r, V, gap, wrap_v):
    """Component number per hit (numbered by first member in find() order): a breadth-first
    closure over the pairwise adjacency, one row of the adjacency matrix at a time."""
    n = len(v)
    comp = np.full(n, -1, dtype=np.int64)

    def neighbours(i):
        dv = np.abs(v - v[i])
        if wrap_v:
            dv = np.minimum(dv, V - dv)
        return np.flatnonzero((dv <= gap[0]) & (np.abs(r - r[i]) <= gap[1]))

    k = 0
    for s in range(n):
        if comp[s] >= 0:
            continue
        comp[s] = k
        q = deque([s])
        while q:
            i = q.popleft()
            for j in neighbours(i):
                if comp[j] < 0:
                    comp[j] = k
                    q.append(j)
        k += 1
    return comp, k


def condense(amp, flag, gap=(1, 1), wrap_v=False):
    """One V x R window.  Returns (peak uint8 [V][R], plots int32 [n][8], (n_plots, n_hits))."""
    flag = np.asarray(flag)
    amp = np.asarray(amp, dtype=np.float32)
    V, R = flag.shape
    v, r = hits(flag)
    comp, k = components(v, r, V, gap, wrap_v)
    peak = np.zeros((V, R), dtype=np.uint8)
    recs = []
    a = amp[v, r]
    for c in range(k):
        m = np.flatnonzero(comp == c)             # in find() order
        i = m[int(np.argmax(a[m]))]               # first maximum
        peak[v[i], r[i]] = 1
        recs.append((r[i] * V + v[i], [v[i], r[i], len(m), v[m].min(), v[m].max(), r[m].min(), r[m].max(), 0]))
    recs.sort(key=lambda t: t[0])
    plots = np.array([t[1] for t in recs], dtype=np.int32).reshape(len(recs), 8)
    return peak, plots, (k, len(v))
