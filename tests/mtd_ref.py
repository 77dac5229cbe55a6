"""A plain fp64 restatement of the MTD stage, its designed scenes and the table of the instance
sweep (tests/test_gpu_mtd_instances.py).  No GPU code and no torch: tests/test_mtd_ref_cpu.py
holds all of it to the oracle without a GPU.

The MTD of one CPI, as the kernels' comments define it (rsp_mtd.hip, mtd_tile):

  pulse p           pc[p] * w[p]
  with an MTI lag   (pc[p + lag] - pc[p]) * w[p], zero from pin - lag on
  Doppler           zero-pad to V, fft along the pulses, magnitude
  fftshift          bin k lands in row (k + V // 2) % V
  zero band         rows of the band are exactly 0: fun_0v_pressing's rows (zero_v_div), or for
                    zero_ends = n the rows [0, n) and [V - n + 1, V)
  two beams         sum |X_L| + |X_R| (zero band applied), difference |X_R| - |X_L| (not zeroed)
"""
import dataclasses

import numpy as np

import rsp_ref as ref

KAISER, HAMMING, RECT = 0, 1, 2      # rsp_params.window
SEED = 20241020


def slow_time_window(kind, pin):
    if kind == RECT:
        return np.ones(pin)
    return ref.hamming(pin) if kind == HAMMING else ref.kaiser(pin, 8.0)


def zero_band(V, zero_v_div=0, zero_ends=0):
    """[V] bool: the rows the MTD writes as exact zeros."""
    z = np.zeros(V, bool)
    if zero_ends > 0:
        z[:zero_ends] = True
        z[V - zero_ends + 1:] = True
    elif zero_v_div:
        a, b = ref.zero_v_rows(V, zero_v_div)
        z[a:b] = True
    return z


def _beam(pc, w, V, shift, mti_lag):
    pc = np.asarray(pc, np.complex128)
    pin = pc.shape[0]
    if mti_lag > 0:
        x = np.zeros_like(pc)
        x[:pin - mti_lag] = pc[mti_lag:] - pc[:pin - mti_lag]
    else:
        x = pc
    x = x * np.asarray(w, np.float64)[:, None]
    pad = np.zeros((V, pc.shape[1]), np.complex128)
    pad[:pin] = x
    mag = np.abs(np.fft.fft(pad, axis=0))
    if shift:
        out = np.empty_like(mag)
        out[(np.arange(V) + V // 2) % V] = mag
        return out
    return mag


def mtd_ref(pc, window, V, shift, zero_band, mti_lag=0, beams=1):   # noqa: A002
    """pc: complex [pin, R] (one beam) or [2, pin, R]; window [pin]; zero_band [V] bool.
    One beam: the RDM plane [V, R].  Two beams: (sum, difference)."""
    zb = np.asarray(zero_band, bool)
    if beams == 1:
        out = _beam(pc, window, V, shift, mti_lag)
        out[zb] = 0.0
        return out
    left = _beam(pc[0], window, V, shift, mti_lag)
    right = _beam(pc[1], window, V, shift, mti_lag)
    s = left + right
    s[zb] = 0.0
    return s, right - left


def beam_magnitudes(pc, window, V, shift, mti_lag=0):
    """(|X_L|, |X_R|) of a two-beam CPI, unzeroed (the scale of the difference plane's bar)."""
    return _beam(pc[0], window, V, shift, mti_lag), _beam(pc[1], window, V, shift, mti_lag)


# ------------------------------------------------------------------------------------ scenes
def _c64(x):
    return np.ascontiguousarray(x.astype(np.complex64))


def _cnoise(rng, shape, sigma=1.0):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * (sigma / np.sqrt(2.0))


def noise(pin, R, seed):
    """Unit-variance complex Gaussian rows [pin, R]."""
    return _c64(_cnoise(np.random.default_rng(seed), (pin, R)))


def tone_bins(V, R):
    """Doppler bin of every column's tone: the edge bins first, then (7 r + 3) % V."""
    k = (7 * np.arange(R) + 3) % V
    if V % 2:
        fold = [(V - 1) // 2 - 1, (V - 1) // 2, (V + 1) // 2]
    else:
        fold = [V // 2 - 1, V // 2, V // 2 + 1]
    forced = []
    for b in [0, 1] + fold + [V - 1]:
        if b % V not in forced:
            forced.append(b % V)
    forced = forced[:R]
    k[:len(forced)] = forced
    return k


def tones(pin, R, V, shift, seed):
    """Column r: a_r exp(2j pi k_r p / V), a_r in [0.5, 2], over a noise floor of 1e-3.
    Returns (rows [pin, R], the RDM row each column's peak must land on)."""
    rng = np.random.default_rng(seed)
    k = tone_bins(V, R)
    a = rng.uniform(0.5, 2.0, R)
    p = np.arange(pin)[:, None]
    x = a[None, :] * np.exp(2j * np.pi * ((k[None, :] * p) % V) / V) + _cnoise(rng, (pin, R), 1e-3)
    return _c64(x), ((k + V // 2) % V if shift else k)


def impulse_pulses(pin, R, G, lag=0):
    """The pulse each column's impulse sits on: 0, 1, G - 1, G, pin - 1, the pulses round pin - lag
    with an MTI, then a walk through [0, pin)."""
    first = [0, 1, G - 1, G, pin - 1]
    if lag > 0:
        first += [pin - lag - 1, pin - lag, pin - lag + 1, lag - 1, lag]
    first = [min(max(q, 0), pin - 1) for q in first][:R]
    p = (np.arange(R) * pin) // R
    p[:len(first)] = first
    return p


def impulses(pin, R, G, seed, lag=0):
    """Column r: zero except a_r at pulse p_r (|a_r| in [0.5, 2], any phase).
    Returns (rows [pin, R], p [R], a [R] as stored in complex64)."""
    rng = np.random.default_rng(seed)
    p = impulse_pulses(pin, R, G, lag)
    a = rng.uniform(0.5, 2.0, R) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, R))
    x = np.zeros((pin, R), np.complex128)
    x[p, np.arange(R)] = a
    x = _c64(x)
    return x, p, x[p, np.arange(R)].astype(np.complex128)


PEAK_MARGIN = 1e-3


def peaked_columns(plane, rows, zb, margin=PEAK_MARGIN):
    """[R] bool: columns of a reference plane whose declared row is outside the zero band and
    stands at least `margin` (relative; a hundred times the RDM bar) over every other row, so that
    an RDM within the bar has its argmax there too."""
    R = plane.shape[1]
    cols = np.arange(R)
    peak = plane[rows, cols]
    rest = plane.copy()
    rest[rows, cols] = -1.0
    return ~np.asarray(zb)[rows] & (peak >= (1.0 + margin) * rest.max(axis=0)) & (peak > 0)


def cpis(case, beams=None):
    """The three CPIs of a case -- noise, tones, impulses -- as complex64 [3, (beams,) pin, R], with
    the tones' declared rows and the impulses' (p, a) of beam 0."""
    nb = case.beams if beams is None else beams
    out, rows, pa = [], None, None
    for b in range(nb):
        s = SEED + 1000 * b
        t, rows_b = tones(case.pin, case.R, case.V, case.shift, s + 1)
        i, p, a = impulses(case.pin, case.R, case.G, s + 2, case.lag)
        if b == 0:
            rows, pa = rows_b, (p, a)
        out.append(np.stack([noise(case.pin, case.R, s + case.seed_off), t, i]))
    x = np.stack(out, axis=1)                         # [3, beams, pin, R]
    return (x[:, 0] if nb == 1 else x), rows, pa


# --------------------------------------------------------------------------------- the sweep
@dataclasses.dataclass(frozen=True)
class Case:
    """One point of the sweep.  V = 0: no zero padding.  G: threads per range bin of the instance
    (V / 16, or V / 24 for the 3 * 2^k lengths; Bluestein: NF / 16), where the scenes put edges."""
    id: str
    pin: int
    R: int
    G: int
    window: int = KAISER
    shift: int = 1
    zdiv: int = 0          # the MTD's zero_v_div
    zends: int = 0         # the MTD's zero_ends
    nfft: int = 0
    beams: int = 1
    lag: int = 0
    methods: tuple = (0, 0)
    seed_off: int = 0      # moved where a seed fails the conditions of test_mtd_ref_cpu.py

    @property
    def V(self):
        return self.nfft or self.pin

    @property
    def cfar_zdiv(self):
        """main_cfar's own zero rows (its /20 band) on the cases whose RDM is shifted."""
        return 20 if self.shift and not self.zends else 0

    def band(self):
        return zero_band(self.V, self.zdiv, self.zends)

    def w(self):
        return slow_time_window(self.window, self.pin)


W57, W32 = (5, 7), (3, 2)
CFAR_T = 3.0


def cfar_windows(case):
    """The CFAR runs a case can hold, as (name, (refV, saveV, refR, saveR)): the Doppler band of
    V - 1 rows and the row of R cells must each hold 2 * (ref + guard) cells (rsp_cfar_params), so
    the 5 + 7 Doppler window needs V >= 25 and takes the 3 + 2 range window where R < 24, and the
    3 + 2 run needs V >= 11.  An MTI lag of pin - 1 leaves one live pulse, a flat plane: no CFAR."""
    out = []
    if case.lag and case.lag == case.pin - 1:
        return out      # one live pulse: every column is flat, nothing to detect
    small = W32 if case.R >= 10 else (1, 0)      # (the two-beam 2048 tile: R = 2 * 2 + 5 = 9)
    if case.V >= 25:
        out.append(("w57", W57 + (W57 if case.R >= 24 else small)))
    if case.V >= 11:
        out.append(("w32", W32 + small))
    return out


def _rot(i):
    """Window, fftshift and zero band rotate across the rows at different periods."""
    return dict(window=(KAISER, HAMMING, RECT)[i % 3], shift=(1, 0)[i % 2],
                **(dict(zdiv=150), dict(), dict(zends=3), dict(zdiv=150))[i % 4],
                methods=((0, 0), (1, 1), (0, 1), (1, 0))[i % 4])


def _cases():
    out = []
    n = [0]

    def add(cid, pin, R, G, **kw):
        d = _rot(n[0])
        n[0] += 1
        if kw.get("nfft", pin) < 8 or pin < 8:     # a band of 3 + 2 rows does not fit
            d.pop("zends", None)
        d.update(kw)
        out.append(Case(cid, pin, R, G, **d))

    # ---- A. every radix instance, one beam, R = 2 W + 5;  B. W < 32: R = 32 W and 64 W
    for P, W, G in ((16, 256, 1), (32, 128, 2), (48, 128, 2), (64, 64, 4), (96, 64, 4), (128, 32, 8), (192, 32, 8),
                    (256, 16, 16), (384, 16, 16), (512, 16, 32), (768, 8, 32), (1024, 16, 64), (1536, 4, 64),
                    (2048, 8, 128)):
        add("a-p%d" % P, P, 2 * W + 5, G)
        if W < 32:
            add("b-p%d-x32" % P, P, 32 * W, G)
            add("b-p%d-x64" % P, P, 64 * W, G)
    # ---- C. zero-padded, one beam
    for (pin, V), W, G in (((33, 64), 64, 4), ((100, 128), 32, 8), ((257, 512), 16, 32), ((1000, 1024), 16, 64),
                           ((1025, 2048), 8, 128), ((1536, 2048), 8, 128)):
        add("c-p%d-v%d" % (pin, V), pin, 2 * W + 5, G, nfft=V)
    # ---- D. two beams (256 threads whatever V): an edge R and one remap R each
    for (pin, V), W, G, RB in (((512, 512), 8, 32, 256), ((300, 512), 8, 32, 512), ((1024, 1024), 4, 64, 128),
                               ((1536, 2048), 2, 128, 128)):
        add("d-p%d-v%d" % (pin, V), pin, 2 * W + 5, G, nfft=V, beams=2)
        add("d-p%d-v%d-x%d" % (pin, V, RB // W), pin, RB, G, nfft=V, beams=2)
    # ---- E. Bluestein: the ends of every transform length's range of P
    for P, W, G in ((2, 64, 4), (17, 64, 4), (31, 64, 4), (33, 32, 8), (63, 32, 8), (65, 16, 16), (127, 16, 16),
                    (129, 16, 32), (255, 16, 32), (257, 16, 64), (511, 16, 64), (513, 8, 128), (1023, 8, 128)):
        add("e-p%d" % P, P, 2 * W + 5, G)
    # ---- F. the fused MTI
    for P, W, G in ((32, 128, 2), (256, 16, 16), (768, 8, 32), (2048, 8, 128), (129, 16, 32)):
        for lag in (1, 9, P - 1):
            add("f-p%d-lag%d" % (P, lag), P, 2 * W + 5, G, lag=lag)
    # ---- B. the other remap branch of the two-beam 1024 and 2048 tiles (512 has both above)
    add("b-p1024-v1024-x64-beams2", 1024, 256, 64, nfft=1024, beams=2)
    add("b-p1536-v2048-x32-beams2", 1536, 64, 128, nfft=2048, beams=2)
    return out


CASES = _cases()

# G. the window stream: (P, W, G) by win; two frame pairs each
WINDOW_CASES = [(P, W, G, win) for P, W, G in ((32, 128, 2), (384, 16, 16), (1024, 16, 64)) for win in (3, 16)]


def window_starts(P, win):
    return [int(np.floor(i * P / win + 0.5)) for i in range(win)]
