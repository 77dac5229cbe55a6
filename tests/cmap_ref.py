"""A plain fp64 restatement of the clutter-map stage (rsp_cmap_dev, include/rsp.h) and its
designed scene.  No GPU code and no torch: tests/test_cmap_cpu.py holds it to hand-computed
recursions, tests/test_gpu_cmap.py holds the kernels to it.

  band amplitude   the unzeroed MTD magnitudes (mtd_ref._beam) picked at the band's rows,
                   summed over the beams
  recursion        per CPI, in order, with m = map[slot], n = age[slot]:
                     flag = n >= max(warmup, 1) and a >= T * m
                     m'   = a                 when n == 0
                     m'   = m                 when hold and flag
                     m'   = m + w * (a - m)   otherwise
                     age  = min(n + 1, AGE_MAX)
                   a CPI with slot < 0 (or >= slots) gets zero flags and touches nothing
"""
import numpy as np

import mtd_ref

AGE_MAX = 2 ** 31 - 1
NEAR_TOL = 1e-5          # |a - T m| / (T m) below this: the cell is near-threshold
F = 12                   # frames of the designed scene
TONE_FROM, TONE_FRAMES = 8, 4


def rows(q_lo, q_hi, V, fftshift):
    """The RDM row of each signed bin q_lo..q_hi."""
    q = np.arange(q_lo, q_hi + 1)
    return (q + V // 2) % V if fftshift else q % V


def band(pc, window, V, q_lo, q_hi, beams=1):
    """pc complex [pin, R] (one beam) or [2, pin, R]; window [pin] -> fp64 [K, R]."""
    r = rows(q_lo, q_hi, V, 0)
    if beams == 1:
        return mtd_ref._beam(pc, window, V, 0, 0)[r]
    return mtd_ref._beam(pc[0], window, V, 0, 0)[r] + mtd_ref._beam(pc[1], window, V, 0, 0)[r]


def recursion(a, T, w, warmup, hold, slot=None, slots=1, state=None):
    """a: [F, K, R] band amplitudes of consecutive CPIs; slot: [F] or None (all 0).
    Returns (flag uint8 [F, K, R], map [slots, K, R], age int64 [slots], margin [F, K, R]) with
    margin = |a - T m| / (T m) where the comparison was made (inf elsewhere).  state: (map, age)
    to start from (not modified)."""
    a = np.asarray(a, np.float64)
    nf, K, R = a.shape
    if state is None:
        m, age = np.zeros((slots, K, R)), np.zeros(slots, np.int64)
    else:
        m, age = np.array(state[0], np.float64), np.array(state[1], np.int64)
    flag = np.zeros((nf, K, R), np.uint8)
    margin = np.full((nf, K, R), np.inf)
    warm = max(int(warmup), 1)
    for f in range(nf):
        s = 0 if slot is None else int(slot[f])
        if s < 0 or s >= slots:
            continue
        n = int(age[s])
        if n >= warm:
            thr = T * m[s]
            fl = a[f] >= thr
            with np.errstate(divide="ignore", invalid="ignore"):
                margin[f] = np.where(thr > 0, np.abs(a[f] - thr) / thr, np.inf)
        else:
            fl = np.zeros((K, R), bool)
        if n == 0:
            m[s] = a[f]
        else:
            upd = m[s] + w * (a[f] - m[s])
            m[s] = np.where(fl, m[s], upd) if hold else upd
        flag[f] = fl
        age[s] = min(n + 1, AGE_MAX)
    return flag, m, age, margin


# ------------------------------------------------------------------------------------ the scene
def tone_plan(R, q_lo, q_hi, bins_per_pass):
    """[(bin, column)]: tones at q_lo, q_hi and the bin each side of every bin-group boundary, dealt
    round the three clutter-free columns (first, last, one in the middle)."""
    bins = [q_lo, q_hi]
    for g in range(q_lo + bins_per_pass, q_hi + 1, bins_per_pass):
        bins += [g - 1, g]
    bins = sorted(set(bins))
    free = free_columns(R)
    return [(q, free[i % len(free)]) for i, q in enumerate(bins)]


def clutter_phase(R):
    """Clutter sits in the columns r % 3 == c, c chosen so that the first and last column are free."""
    return 2 if (R - 1) % 3 == 1 else 1


def free_columns(R):
    c = clutter_phase(R)
    mid = R // 2
    while mid % 3 == c:
        mid += 1
    out = []
    for r in (0, R - 1, min(mid, R - 1)):
        if r not in out:
            out.append(r)
    return out


def scene(P, V, R, q_lo, q_hi, window, beams=1, bins_per_pass=16, seed=0, clutter=30.0):
    """F frames of complex64 rows [F, (beams,) P, R]: unit noise, stationary zero-Doppler clutter
    of amplitude `clutter` in every third column with a 5 % frame-to-frame scale, and from frame
    TONE_FROM on, for TONE_FRAMES frames, the tones of tone_plan.  A tone's amplitude is
    24 sqrt(sum w^2) / sum w: its band cell stands at 24 noise sigmas of the filter, three times
    the 2 T = 8 the tests ask for at T = 4.  Returns (rows, [(k, column)] of the tone cells)."""
    rng = np.random.default_rng(mtd_ref.SEED + seed)
    win = mtd_ref.slow_time_window(window, P)
    amp = 24.0 * np.sqrt(np.sum(win ** 2)) / np.sum(win)
    p = np.arange(P)
    cl = np.where(np.arange(R) % 3 == clutter_phase(R), clutter, 0.0) * np.exp(2j * np.pi * rng.uniform(size=R))
    plan = tone_plan(R, q_lo, q_hi, bins_per_pass)
    out = np.empty((F, beams, P, R), np.complex64)
    for f in range(F):
        scale = 1.0 + 0.05 * rng.standard_normal()
        for b in range(beams):
            x = (rng.standard_normal((P, R)) + 1j * rng.standard_normal((P, R))) / np.sqrt(2.0)
            x += cl[None, :] * scale
            if TONE_FROM <= f < TONE_FROM + TONE_FRAMES:
                for q, col in plan:
                    x[:, col] += amp * np.exp(2j * np.pi * ((q * p) % V) / V)
            out[f, b] = x
    cells = [(q - q_lo, col) for q, col in plan]
    return (out[:, 0] if beams == 1 else out), cells


def scene_band(x, window, P, V, q_lo, q_hi, beams):
    """fp64 band amplitudes [F, K, R] of a scene's rows."""
    win = mtd_ref.slow_time_window(window, P)
    return np.stack([band(x[f], win, V, q_lo, q_hi, beams) for f in range(x.shape[0])])


# --------------------------------------------------------------------------------- the sweep
# The smallest shapes that reach every band kernel instance rsp_cmap_plan can report
# (bins_per_pass 4 / 16 x vec 1 / 2 x split 1 / 4): id, P, V, beams, (q_lo, q_hi), R, ld, window,
# w, and the instance the plan must report.  split = 4 needs P >= 256 and R <= 1024, vec = 2 an
# even R and ld, 16 bins per pass K > 4; R = 130 and 200 span more than one 64-thread workgroup
# of two columns per thread, R = 1100 is the one P >= 256 shape past the split's R.
CASES = [
    ("p2-k1-r1", 2, 2, 1, (0, 0), 1, 1, mtd_ref.RECT, 0.25, (4, 1, 1)),
    ("p16-k3-r130", 16, 16, 1, (-2, 0), 130, 130, mtd_ref.HAMMING, 0.125, (4, 2, 1)),
    ("p33v64-k7-r69", 33, 64, 1, (-3, 3), 69, 69, mtd_ref.KAISER, 0.25, (16, 1, 1)),
    ("p128-k13-r200-ld208", 128, 128, 1, (-7, 5), 200, 208, mtd_ref.KAISER, 0.125, (16, 2, 1)),
    ("p332-k17-r67", 332, 332, 1, (-8, 8), 67, 67, mtd_ref.HAMMING, 0.25, (16, 1, 4)),
    ("p332-k3-r66", 332, 332, 1, (-1, 1), 66, 66, mtd_ref.RECT, 0.125, (4, 2, 4)),
    ("p332-k1-r65-ld71", 332, 332, 1, (1, 1), 65, 71, mtd_ref.KAISER, 0.25, (4, 1, 4)),
    ("p1536v2048-k64-r70-ld72-beams2", 1536, 2048, 2, (-32, 31), 70, 72, mtd_ref.HAMMING, 0.125, (16, 2, 4)),
    ("p332-k13-r1100", 332, 332, 1, (-6, 6), 1100, 1100, mtd_ref.KAISER, 0.25, (16, 2, 1)),
]
T = 4.0
WARMUP = 4


def case_scene(case):
    """(rows [F, (beams,) P, R] complex64, tone cells, fp64 band [F, K, R]) of a sweep case."""
    cid, P, V, beams, (q_lo, q_hi), R, ld, window, w, inst = case
    x, cells = scene(P, V, R, q_lo, q_hi, window, beams, bins_per_pass=inst[0], seed=len(cid))
    return x, cells, scene_band(x, window, P, V, q_lo, q_hi, beams)
