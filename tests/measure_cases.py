"""The designed cases of the hit-list / measurement sweep (tests/test_gpu_measure_sweep.py) and
their scene builders.  No GPU imports: tests/test_measure_cases_cpu.py checks on the CPU, against
the oracle alone, that every row takes the plan it names and that its scene holds what the row is
for; tests/test_measplan_cpu.py checks the plans against the library's own answer.

A row is the smallest shape at which a branch of hits_kernel (csrc/rsp_measure.hip) exists.  One
pass of its column loop covers G * cw columns (16384 on the 16-byte path, 1024 on the byte path
at G = 1024); slice s of S = 1024 / G owns rows min(V, s*rows) .. min(V, (s+1)*rows) with
rows = ceil(V / S), and a thread keeps one mask bit per q = ceil(rows / 64) rows.

Every case is a batch of 3 CPIs with different scenes.  The planes are windows: R columns from
column col0 of rows ld elements apart, CPIs cs = V * ld + pad elements apart, inside buffers whose
every other element (other columns, the CPI padding, 64 elements before and after) holds a 3e30
amplitude and a set flag, so a read outside the window shows.  rScale and vScale are random fp64,
not linear, so that a wrong index cannot cancel.
"""
import numpy as np

import measure_ref as mr

BATCH = 3
GUARD = 64                      # elements before and after the planes
OUTSIDE_AMP = np.float32(3.0e30)
HIT_BYTES = (1, 2, 0x7F, 0x80, 0xFF)
RUN = (0x80, 0x01, 0x00, 0xFF, 0x7F, 0x00)      # straddles a 4-byte boundary wherever it starts
FIXED = dict(delta_r=5.996, delta_v=0.371, k_value=10.880367, beam_pos_num=5, beam_angle_step=5.0, ele_comp=0.125,
             ele_sys_err=-0.5)


def geometry(V, R, ld, cs, addr):
    """The hit-list geometry restated from the kernel's description (one band)."""
    wide = R % 16 == 0 and R >= 256 and ld % 16 == 0 and cs % 16 == 0 and addr % 16 == 0
    cw = 16 if wide else 1
    G = 16 if wide else 64
    while G < -(-R // cw) and G < 1024:
        G *= 2
    S = 1024 // G
    rows = -(-V // S)
    return dict(wide=wide, G=G, S=S, rows=rows, q=-(-rows // 64), passes=-(-R // (G * cw)))


def wide_terms(c):
    """The five terms of the `wide` predicate for a case whose buffers start 16-byte aligned."""
    return dict(r16=c.R % 16 == 0, r256=c.R >= 256, ld=c.ld % 16 == 0, cs=c.cs % 16 == 0, ptr=c.col0 % 16 == 0)


class Case:
    def __init__(self, id, V, R, plan, hits, col0=0, ld=None, pad=0, e=2, M0=1, interp=(8, 4), max_hits=None,
                 flags="sparse", amps="random", density=0.0, extra=(), seed=0, marks=(), what="",
                 scales=(2000.0, 40.0)):
        self.id, self.V, self.R, self.col0, self.pad = id, V, R, col0, pad
        self.ld = R if ld is None else ld
        self.cs = V * self.ld + pad
        self.e, self.M0, self.interp = e, M0, interp
        self.flags, self.amps, self.density, self.extra, self.seed = flags, amps, density, tuple(extra), seed
        self.plan = dict(zip(("wide", "G", "S", "rows", "q", "passes"), plan))
        self.hits = hits                                    # (lo, hi): the hit count of every CPI lies in it
        self.max_hits = hits[1] + 7 if max_hits is None else max_hits
        self.marks, self.what, self.batch = frozenset(marks), what, BATCH
        self.scales = scales                                # magnitudes of the random rScale / vScale

    def __repr__(self):
        return "Case(%s)" % self.id


def _tight(e, M0):
    # R = 2e+1 and V - 2*M0 - 1 = 2e+1: the only cells a hit can be measured on, and every cell flagged
    V, R = 2 * e + 2 + 2 * M0, 2 * e + 1
    return Case("tight-e%d-m%d" % (e, M0), V, R, (False, 64, 16, 1, 1, 1), (V * R, V * R), e=e, M0=M0, flags="all",
                amps="random" if M0 == 0 else "extremes", max_hits=V * R + 5, seed=40 + 10 * e + M0,
                marks=("all",) + (("extremes",) if M0 else ()),
                what="every hit re-anchors to the same cells; all cells flagged; max_hits > V*R")


_WIN = dict(ld=304, pad=32)
# two rows of one mask bit (0|1, 198|199), several bits of one thread (rows 0, 10, 31, 65 of slice 0), the last
# slice's last row, several columns of one thread's 16
_Q2_EXTRA = ((0, 5), (1, 5), (1, 7), (10, 5), (31, 6), (65, 5), (66, 5), (198, 5), (199, 5), (260, 4095), (259, 4080),
             (260, 4081), (131, 2048), (130, 2049))

CASES = [
    Case("w-min", 8, 256, (True, 16, 64, 1, 1, 1), (40, 100), e=1, M0=1, density=0.03, amps="extremes", seed=1,
         marks=("extremes",), what="V < S: 56 empty slices"),
    Case("w-ragged", 130, 256, (True, 16, 64, 3, 1, 1), (90, 190), e=2, M0=5, density=0.004, amps="plateau", seed=2,
         extra=((129, 0), (129, 100), (129, 255), (128, 17), (126, 17)), marks=("plateau",),
         what="last used slice (43) has 1 row, later ones none"),
    Case("w-q2", 261, 4096, (True, 256, 4, 66, 2, 1), (120, 200), e=2, M0=5, interp=(16, 2), density=0.00013, seed=3,
         extra=_Q2_EXTRA, marks=("q2",), what="hits in two rows of one mask bit and in several bits of one thread"),
    Case("w-2pass", 8, 16400, (True, 1024, 1, 8, 1, 2), (120, 200), e=1, M0=1, density=0.001, flags="bytes", seed=4,
         extra=((3, 16383), (3, 16384), (0, 16399), (7, 16399), (4, 16390), (5, 16385)),
         what="second pass has one 16-column group; hits in both passes and in the last 16 columns"),
    Case("w-window", 40, 256, (True, 16, 64, 1, 1, 1), (110, 200), col0=16, e=2, M0=3, density=0.014, flags="bytes",
         seed=5, what="wide with ld > R: strides on the 16-byte path", **_WIN),
    Case("b-col7", 40, 256, (False, 256, 4, 10, 1, 1), (110, 200), col0=7, e=2, M0=3, density=0.014, flags="bytes",
         seed=6, what="pointer alignment alone turns wide off", **_WIN),
    Case("b-ld", 40, 256, (False, 256, 4, 10, 1, 1), (110, 200), ld=300, e=2, M0=3, density=0.014, amps="extremes",
         seed=7, marks=("extremes",), what="pitch alone"),
    Case("b-cs", 40, 256, (False, 256, 4, 10, 1, 1), (110, 200), pad=8, e=2, M0=3, density=0.014, seed=8,
         what="CPI stride alone"),
    Case("b-240", 40, 240, (False, 256, 4, 10, 1, 1), (100, 190), e=2, M0=3, density=0.014, amps="plateau", seed=9,
         marks=("plateau",), what="R % 16 == 0 but < 256"),
    Case("b-2pass", 8, 1030, (False, 1024, 1, 8, 1, 2), (120, 200), e=1, M0=1, density=0.018, seed=10,
         extra=((0, 1024), (7, 1029), (3, 1026), (4, 1023)), what="6 columns in the last pass"),
    Case("b-3pass", 8, 2055, (False, 1024, 1, 8, 1, 3), (150, 200), e=1, M0=1, density=0.0105, max_hits=60, seed=11,
         extra=((0, 1500), (0, 1024), (0, 2050), (5, 2048), (0, 2054)), marks=("cut",),
         what="base carried twice; the cut lies in pass 1, passes 2 and 3 are count-only and their failing hits "
              "reach count[:, 1]"),
    Case("b-1025", 12, 1025, (False, 1024, 1, 12, 1, 2), (110, 200), e=2, M0=3, density=0.011, seed=12,
         extra=((0, 1024), (5, 1024), (6, 1024), (11, 1024)), what="last pass is one column, and it holds hits"),
]
CASES += [_tight(e, M0) for e in (1, 2, 3, 4) for M0 in (0, 3)]
# The interp and e-all rows are there for the last bit of the spline's abscissae.  One ulp of a cell index is
# some 1e-15 in an estimate, so their scales are small (a scale of hundreds would round it away: the rows
# would pass with a wrong colon), and their hits crowd the low cells, where MATLAB's two halves differ.
_ULP = dict(flags="low", M0=0, scales=(1e-3, 1e-3), marks=("interp",))
CASES += [Case("interp-%d-%d" % f, 48, 300, (False, 512, 2, 24, 1, 1), (130, 230), e=2, interp=f, density=0.004,
               seed=60, what="the b-side of the colon, on the GPU", **_ULP)
          for f in ((1, 1), (3, 5), (7, 10), (63, 64), (6, 12))]   # seed: the first that gives every CPI such a hit
CASES += [Case("e-all-%d" % e, 64, 272, (True, 32, 32, 2, 1, 1), (130, 250), e=e, interp=(5, 3), density=0.002,
               seed=80 + e, what="measure_kernel<%d> with an inexact step" % e, **_ULP) for e in (1, 2, 3, 4)]
BY_ID = {c.id: c for c in CASES}


# ---------------------------------------------------------------------------------- scene builders
def _flags(c, rng):
    V, R = c.V, c.R
    if c.flags == "all":
        return np.ones((BATCH, V, R), np.uint8)
    m = rng.random((BATCH, V, R)) < c.density
    if c.flags == "low":
        # many hits whose cells start at 1..8: only there does the half of MATLAB's colon that counts down
        # from b differ from a + i*d for steps as coarse as 1/5 and 1/10 (the sums are exact further up)
        m[:, :6, :] |= rng.random((BATCH, 6, R)) < 0.035
        m[:, :, :8] |= rng.random((BATCH, V, 8)) < 0.16
    # the corner and edge hits of test_gpu_measure.py's _scene
    m[:, 0, 0] = m[:, V - 1, R - 1] = m[:, 0, R - 1] = m[:, V - 1, 0] = True
    m[:, V // 2, 0] = m[:, V // 2, R - 1] = True
    for v, r in c.extra:
        m[:, v, r] = True
    if c.flags in ("sparse", "low"):
        return m.astype(np.uint8)
    # "bytes": any nonzero byte is a hit
    f = np.where(m, rng.choice(np.array(HIT_BYTES, np.uint8), size=m.shape), 0).astype(np.uint8)
    starts = [2, 13, 29, 61, R // 2 - 3, R - 6]             # across 4- and 16-byte boundaries; the last columns
    if c.plan["passes"] > 1:
        starts.append(c.plan["G"] * (16 if c.plan["wide"] else 1) - 3)     # across the pass boundary
    for b in range(BATCH):
        for k, s0 in enumerate(starts):
            f[b, (b + 2 * k + 1) % V, s0:s0 + len(RUN)] = RUN
    for v, r in c.extra:                                    # a run's zero may have landed on a designed hit
        f[:, v, r] = np.where(f[:, v, r] == 0, 0x80, f[:, v, r])
    return f


def _amps(c, rng, f):
    V, R, e = c.V, c.R, c.e
    s = (rng.random((BATCH, V, R)) * 2 + 0.1).astype(np.float32)
    d = (rng.standard_normal((BATCH, V, R)) * 0.5).astype(np.float32)
    if c.amps == "plateau":
        # round every hit in turn: a block of equal values (both maxima are ties), a block of exact zeros with
        # a zero difference (0/0), a block of zeros with the difference kept (x/0), or nothing
        for b in range(BATCH):
            for k, (r, v) in enumerate(zip(*np.nonzero(f[b].T))):
                kind = k % 4
                if kind == 3:
                    continue
                blk = (b, slice(max(v - 2 * e, 0), v + 2 * e + 1), slice(max(r - 2 * e, 0), r + 2 * e + 1))
                s[blk] = np.float32(1.5) if kind == 0 else np.float32(0.0)
                if kind == 1:
                    d[b, v, r] = 0.0
    elif c.amps == "extremes":
        # fp32 extremes next to ordinary values: finite, so no estimate but the elevation can be non-finite
        u = rng.random((BATCH, V, R))
        s[u < 0.12] = np.float32(1e-38)
        s[u > 0.88] = np.float32(3e38)
        w = rng.random((BATCH, V, R))
        d[w < 0.05] = np.float32(-3e38)
        d[w > 0.95] = np.float32(1e-38)
    return s, d


class Scene:
    def __init__(self, c):
        rng = np.random.default_rng(1000 + c.seed)
        self.case = c
        self.f = _flags(c, rng)
        self.s, self.d = _amps(c, rng, self.f)
        self.r_scale = (rng.random(c.R) * 2000.0 - 300.0) * (c.scales[0] / 2000.0)
        self.v_scale = rng.standard_normal(c.V) * c.scales[1]
        self.kw = dict(FIXED, extra_dots=c.e, r_interp=c.interp[0], v_interp=c.interp[1], mtd0_num=c.M0,
                       r_scale=self.r_scale, v_scale=self.v_scale)
        self._oracle = None

    def oracle(self):
        """Per CPI: (est [n][3] float64, cells [n][2]) of all hits, failed ones NaN (computed once)."""
        if self._oracle is None:
            out = []
            for b in range(BATCH):
                re, ve, el, hc = mr.motion_para_measure(self.s[b].astype(np.float64), self.d[b].astype(np.float64),
                                                        self.f[b], on_error="nan", **self.kw)
                out.append((np.stack([re, ve, el], axis=1).reshape(-1, 3), hc))
            self._oracle = out
        return self._oracle

    def index(self, first_cpi=0, n=BATCH):
        """Element indices [n][V][R] of the windows of CPIs first_cpi.. in the buffers."""
        c = self.case
        b = np.arange(first_cpi, first_cpi + n)[:, None, None]
        return GUARD + b * c.cs + np.arange(c.V)[None, :, None] * c.ld + c.col0 + np.arange(c.R)[None, None, :]

    def buffers(self):
        """(sum, diff, flag) flat host buffers: the windows inside, 3e30 and set flags everywhere else."""
        c = self.case
        n = GUARD + BATCH * c.cs + GUARD
        s = np.full(n, OUTSIDE_AMP, np.float32)
        d = np.full(n, OUTSIDE_AMP, np.float32)
        f = np.full(n, 0xFF if c.flags == "bytes" else 1, np.uint8)
        idx = self.index()
        s[idx], d[idx], f[idx] = self.s, self.d, self.f
        return s, d, f


_SCENES = {}


def scene(c):
    if c.id not in _SCENES:
        _SCENES[c.id] = Scene(c)
    return _SCENES[c.id]
