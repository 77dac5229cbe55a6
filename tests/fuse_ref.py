"""Restatement of rsp_beam_fuse_dev / rsp_beam_elev_dev (include/rsp.h: stacked beams fused per cell,
elevation from the beam amplitudes), for the tests: numpy, statement for statement.

    fuse(amp, flag, min_beams) -> (fflag, fbeam, famp, fcnt)
    elev_one(law, k, x, am, a0, ap) -> (el, three)
    elevation(amp, flag, fbeam, cells, count, beam_el, law) -> (el [batch][max_hits], hb [batch][max_hits][4])

amp is float32 [batch][beams][V][R], flag uint8 of the same shape (any nonzero byte is a hit).  The
compares are float32 `>` in beam order, the elevation is fp64 in the stated operation order.  Written for
clarity, not speed.
"""
import math

import numpy as np


def fuse(amp, flag, min_beams):
    amp = np.asarray(amp, dtype=np.float32)
    flag = np.asarray(flag, dtype=np.uint8)
    B, K, V, R = amp.shape
    m = amp[:, 0].copy()
    cnt = np.zeros((B, V, R), np.int32)
    best = np.zeros((B, V, R), np.float32)
    k_best = np.full((B, V, R), 255, np.int32)
    for k in range(K):
        a, f = amp[:, k], flag[:, k] != 0
        if k > 0:
            m = np.where(a > m, a, m)
        cnt += f
        take = f & ((k_best == 255) | (a > best))     # `>`: the first of equal amplitudes wins
        best = np.where(take, a, best)
        k_best = np.where(take, k, k_best)
    hit = cnt >= int(min_beams)
    fflag = hit.astype(np.uint8)
    fbeam = np.where(hit, k_best, 255).astype(np.uint8)
    return fflag, fbeam, m.astype(np.float32), cnt.astype(np.uint8)


def elev_one(law, k, x, am, a0, ap, log=math.log):
    """The rule for one hit whose peak beam is k (not 255): x the beam centres, am / a0 / ap the float32
    amplitudes of beams k-1, k, k+1 (am / ap are not looked at where they do not exist).  Returns (el,
    three): three is True where the three-beam formula gave the result.  `log` lets a test move the
    logarithms by a few ulp."""
    x = [float(v) for v in x]
    x0 = x[k]
    if law == 0 or k == 0 or k == len(x) - 1:
        return x0, False
    xm, xp = x[k - 1], x[k + 1]
    am, a0, ap = float(np.float32(am)), float(np.float32(a0)), float(np.float32(ap))
    if law == 1:
        with np.errstate(all="ignore"):
            wm, w0, wp = np.float64(am) * np.float64(am), np.float64(a0) * np.float64(a0), np.float64(ap) * np.float64(ap)
            num = (wm * xm + w0 * x0) + wp * xp
            den = (wm + w0) + wp
            if den == 0.0 or not np.isfinite(den):
                return x0, False
            return float(num / den), True
    for a in (am, a0, ap):
        if not (a > 0.0) or not math.isfinite(a):
            return x0, False
    ym, y0, yp = log(am), log(a0), log(ap)
    with np.errstate(all="ignore"):
        dm, dp = np.float64(x0) - xm, np.float64(x0) - xp
        A, Bq = np.float64(y0) - yp, np.float64(y0) - ym
        den = dm * A - dp * Bq
        xv = x0 - 0.5 * (dm * dm * A - dp * dp * Bq) / den
        if den * (np.float64(xp) - xm) <= 0.0 or not np.isfinite(xv):
            return x0, False
    lo, hi = min(xm, xp), max(xm, xp)
    return float(lo if xv < lo else (hi if xv > hi else xv)), True


def hit_inputs(amp, flag, fbeam, b, row, col, beams):
    """What the rule reads for the hit at (row, col) of CPI b: (k, flagged beams, am, a0, ap); k is 255
    where d_fbeam says so, holds a beam that does not exist, or the cell lies outside the planes."""
    _, K, V, R = amp.shape
    if not (0 <= row < V and 0 <= col < R):
        return 255, 0, 0.0, 0.0, 0.0
    k = int(fbeam[b, row, col])
    if k >= beams:
        k = 255
    cnt = int((flag[b, :, row, col] != 0).sum())
    if k == 255:
        return 255, cnt, 0.0, 0.0, 0.0
    am = amp[b, k - 1, row, col] if k > 0 else np.float32(0)
    ap = amp[b, k + 1, row, col] if k < beams - 1 else np.float32(0)
    return k, cnt, am, amp[b, k, row, col], ap


def elevation(amp, flag, fbeam, cells, count, beam_el, law, log=math.log):
    """el float64 [batch][max_hits] and hb int32 [batch][max_hits][4]; slots at or past
    min(count[b][0], max_hits) come back as NaN / -9 (the call leaves them untouched)."""
    amp = np.asarray(amp, dtype=np.float32)
    B, K, V, R = amp.shape
    H = cells.shape[1]
    el = np.full((B, H), np.nan)
    hb = np.full((B, H, 4), -9, np.int32)
    for b in range(B):
        for i in range(max(0, min(int(count[b, 0]), H))):
            row, col = int(cells[b, i, 0]), int(cells[b, i, 1])
            k, cnt, am, a0, ap = hit_inputs(amp, flag, fbeam, b, row, col, K)
            if k == 255:
                el[b, i], hb[b, i] = np.nan, (-1, cnt, -1, -1)
                continue
            e, three = elev_one(law, k, beam_el[:K], am, a0, ap, log=log)
            el[b, i] = e
            hb[b, i] = (k, cnt, k - 1 if three else -1, k + 1 if three else -1)
    return el, hb
