"""Restatement of the ordered-statistic CFAR (include/rsp.h, rsp_os_cfar_dev) and the scenes, shapes
and parameter grid that tests/test_oscfar_cpu.py and tests/test_gpu_oscfar.py share.

os_cfar() is written from the rule as it is stated: the reference windows of every cell are
gathered, sorted (np.sort) and the k-th smallest is read; the threshold is one np.float32 product.
It does not use the counting identity the kernels use.  os_cfar_counting() is the second form
(counts of fl32(T * z_i) <= z[y]) and os_line64() the plain fp64 one; the CPU tests hold the three
against each other.

Rows and columns are 0-based, the band is [lo, hi) = [M0 + 1, V - M0), segments are [a, b).
"""
from dataclasses import dataclass

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import cfar_scene
import rsp_ref as ref

GO, SO, UNION = "go", "so", "union"


@dataclass(frozen=True)
class Params:
    refV: int
    saveV: int
    refR: int
    saveR: int
    M0: int
    segments: tuple = ()         # () = the whole row
    zero_v_div: int = 0
    TV: float = 4.0
    TR: float = 4.0
    form: str = GO               # both stages
    kV: int = 1
    kR: int = 1
    rFlag: int = 1

    @property
    def union(self):
        return self.form == UNION

    @property
    def method(self):
        return 1 if self.form == SO else 0


# ---------------------------------------------------------------------------------- the rule
def _windows(Z, lo, hi, ref_, save):
    """For lines Z [n][len] with valid part [lo, hi): the cells y of the valid part, the two windows'
    values [n][cells][ref] and which side fits.  A side that leaves the valid part is replaced by the
    other side (Function_CFAR1D_sub.m:30-39)."""
    sw = sliding_window_view(Z, ref_, axis=1)          # sw[:, s] = Z[:, s : s + ref]
    y = np.arange(lo, hi)
    l1, r1 = y - save - ref_, y + save + 1
    lok, rok = l1 >= lo, r1 + ref_ <= hi
    assert np.all(lok | rok), "both windows leave the valid part"
    Lw = sw[:, np.where(lok, l1, r1)]
    Rw = sw[:, np.where(rok, r1, l1)]
    return y, Lw, Rw, lok, rok


def _kth(W, k):
    return np.sort(W, axis=-1)[..., k - 1]


def os_line(Z, lo, hi, ref_, save, k, form, T):
    """pass [n][len] bool (False off the valid part) and the statistic w [n][len] float32."""
    Z = np.ascontiguousarray(Z, np.float32)
    y, Lw, Rw, _, _ = _windows(Z, lo, hi, ref_, save)
    if form == UNION:
        w = _kth(np.concatenate([Lw, Rw], axis=-1), k)
    else:
        a, b = _kth(Lw, k), _kth(Rw, k)
        w = np.maximum(a, b) if form == GO else np.minimum(a, b)
    thr = np.float32(T) * w.astype(np.float32)
    assert thr.dtype == np.float32
    out = np.zeros(Z.shape, bool)
    out[:, lo:hi] = Z[:, lo:hi] >= thr
    wf = np.zeros(Z.shape, np.float32)
    wf[:, lo:hi] = w
    return out, wf


def os_line_counting(Z, lo, hi, ref_, save, k, form, T):
    """The same decision from the side counts cl, cr of fl32(T * z_i) <= z[y]."""
    Z = np.ascontiguousarray(Z, np.float32)
    TZ = np.float32(T) * Z
    y, Lw, Rw, _, _ = _windows(TZ, lo, hi, ref_, save)
    x = Z[:, lo:hi, None]
    cl, cr = (Lw <= x).sum(-1), (Rw <= x).sum(-1)
    if form == UNION:
        p = cl + cr >= k
    elif form == GO:
        p = (cl >= k) & (cr >= k)
    else:
        p = (cl >= k) | (cr >= k)
    out = np.zeros(Z.shape, bool)
    out[:, lo:hi] = p
    return out


def os_line64(Z, lo, hi, ref_, save, k, form, T):
    """The plain fp64 form, one cell of every line at a time with np.partition: (pass, margin
    |z - T w| / (T w)).  Where
    T w = 0 the test is z >= 0, which holds for every magnitude in any precision: margin inf."""
    Z = np.asarray(Z, np.float64)
    out = np.zeros(Z.shape, bool)
    margin = np.full(Z.shape, np.inf)
    for y in range(lo, hi):                       # one cell of every line at a time
        l1, r1 = y - save - ref_, y + save + 1
        lok, rok = l1 >= lo, r1 + ref_ <= hi
        assert lok or rok
        L = Z[:, l1:l1 + ref_] if lok else Z[:, r1:r1 + ref_]
        Rt = Z[:, r1:r1 + ref_] if rok else Z[:, l1:l1 + ref_]
        if form == UNION:
            w = np.partition(np.hstack([L, Rt]), k - 1, axis=1)[:, k - 1]
        else:
            a, b = np.partition(L, k - 1, axis=1)[:, k - 1], np.partition(Rt, k - 1, axis=1)[:, k - 1]
            w = np.maximum(a, b) if form == GO else np.minimum(a, b)
        thr = float(T) * w
        out[:, y] = Z[:, y] >= thr
        pos = thr > 0
        margin[pos, y] = np.abs(Z[pos, y] - thr[pos]) / thr[pos]
    return out, margin


def _prepare(x, p):
    x = np.array(x, np.float32, copy=True)
    V, R = x.shape
    if p.zero_v_div:
        a, b = ref.zero_v_rows(V, p.zero_v_div)
        x[max(a, 0):b] = 0.0
    return x, p.M0 + 1, V - p.M0, (list(p.segments) or [(0, R)])


def stage_lines(x, p):
    """[(stage, Z, lo, hi, test arguments, place)]: the lines of both stages, for the tests that hold
    the 1-D forms against each other.  place(out) puts a [n][len] result back as a [V][R] map."""
    x, lo, hi, segs = _prepare(x, p)
    V, R = x.shape
    cols = np.zeros(R, bool)
    for a, b in segs:
        cols[a:b] = True

    def place_v(o, cols=cols):
        m = np.zeros((V, R), o.dtype)
        m[:, cols] = o.T
        return m
    out = [("V", x.T[cols], lo, hi, (p.refV, p.saveV, p.kV, p.form, p.TV), place_v)]
    for a, b in segs:
        def place_r(o, a=a, b=b):
            m = np.zeros((V, R), o.dtype)
            m[lo:hi, a:b] = o
            return m
        out.append(("R", x[lo:hi, a:b], 0, b - a, (p.refR, p.saveR, p.kR, p.form, p.TR), place_r))
    return out


def os_cfar(x, p, line=os_line):
    """The whole stage on one [V][R] plane: dict(flag, flagV uint8 [V][R]; passR bool [V][R], the
    range test at every in-segment band cell; moved / dropped bool [V][R], the Doppler hits whose
    flag lands on a neighbour / whose candidates all fail).  `line` is the 1-D form."""
    xz, lo, hi, segs = _prepare(x, p)
    V, R = xz.shape
    flagV = np.zeros((V, R), bool)
    passR = np.zeros((V, R), bool)
    for stage, Z, a, b, args, place in stage_lines(x, p):
        r = line(Z, a, b, *args)
        r = r[0] if isinstance(r, tuple) else r
        if stage == "V":
            flagV |= place(r)
        else:
            passR |= place(r)
    res = dict(flagV=flagV.astype(np.uint8), passR=passR)
    if not p.rFlag:
        res.update(flag=res["flagV"].copy(), moved=np.zeros((V, R), bool), dropped=np.zeros((V, R), bool))
        return res
    flag = np.zeros((V, R), np.uint8)
    moved = np.zeros((V, R), bool)
    dropped = np.zeros((V, R), bool)
    for a, b in segs:
        hv, hr = np.nonzero(flagV[:, a:b])
        hr = hr + a
        if hv.size == 0:
            continue
        q = hr[:, None] + np.array([-1, 0, 1])[None, :]              # the candidates r-1, r, r+1
        inside = (q >= a) & (q < b)                                  # confined to the hit's segment
        qc = np.clip(q, 0, R - 1)
        ok = inside & passR[hv[:, None], qc]
        vals = np.where(ok, xz[hv[:, None], qc], np.float32(-1.0))   # magnitudes are >= 0
        best = np.argmax(vals, axis=1)                               # the first maximum
        has = ok.any(axis=1)
        flag[hv[has], q[has, best[has]]] = 1
        moved[hv[has], hr[has]] = best[has] != 1
        dropped[hv[~has], hr[~has]] = True
    res.update(flag=flag, moved=moved, dropped=dropped)
    return res


def os_cfar_counting(x, p):
    return os_cfar(x, p, line=os_line_counting)


# ---------------------------------------------------------------------------------- scenes
@dataclass(frozen=True)
class Shape:
    name: str
    V: int
    R: int
    ref: int
    save: int
    M0: int
    nseg: int
    batch: int = 1
    zero_v_div: int = 0

    @property
    def segments(self):
        return tuple(cfar_scene.layout(self.R, self.ref + self.save, self.nseg))

    def params(self, form=GO, k=1, rFlag=1, T=4.0):
        return Params(self.ref, self.save, self.ref, self.save, self.M0, self.segments, self.zero_v_div,
                      float(T), float(T), form, int(k), int(k), int(rFlag))


# (V, R, ref, save, M0, segments) of the sweep; the 332-row one carries the zero_v_div band
SHAPES = (Shape("40x40", 40, 40, 2, 1, 0, 0),
          Shape("64x70", 64, 70, 5, 7, 2, 1),
          Shape("332x130", 332, 130, 5, 7, 3, 3, zero_v_div=20),
          Shape("2048x62", 2048, 62, 5, 7, 6, 0, batch=2))
# further Doppler tile widths (the tile is sized by V alone): narrow planes, one case each
TILE_SHAPES = (Shape("256x24", 256, 24, 3, 2, 1, 0),
               Shape("1024x24", 1024, 24, 3, 2, 1, 0),
               Shape("4096x20", 4096, 20, 3, 2, 1, 0))
WIN = dict(V=96, R=130, col0=7, ld=160, cs=96 * 160 + 48, batch=2, ref=5, save=7, M0=2, nseg=3)


def ranks(shape, form):
    """k = 1, the middle rank and the largest rank of the form."""
    n = 2 * shape.ref if form == UNION else shape.ref
    return sorted({1, (n + 1) // 2, n})


def cases(shape):
    """[(form, k, rFlag)] of the sweep."""
    return [(f, k, rf) for f in (GO, SO, UNION) for k in ranks(shape, f) for rf in (0, 1)]


_SCENES = {}


def scene(shape):
    """float32 [batch][V][R]: cfar_scene's designed field (Rayleigh floor of mean 1, spikes of 30-80
    on the cells where the kernels take another branch, a run that passes the Doppler test and fails
    the range test, a re-localisation pair, a block of exact zeros over whole windows where it
    fits), built once per shape and never written to.  Every non-zero value and every product
    T * value is in the normal fp32 range."""
    if shape.name not in _SCENES:
        planes = []
        for b in range(shape.batch):
            sc = cfar_scene.build(shape.V, shape.R, list(shape.segments), shape.M0, shape.zero_v_div, shape.ref,
                                  shape.save, shape.ref, shape.save, seed=cfar_scene.SEED + 17 * b + shape.V)
            x = sc.field.astype(np.float32)
            if shape in SHAPES:       # the narrow tile-width planes have no room for them and no audit
                if shape.name == ZERO_BLOCK_SHAPE and b == 0:
                    _zero_block(x, shape)
                _run(x, shape)
                _edge_spikes(x, shape)
            planes.append(x)
        a = np.stack(planes)
        nz = a[a != 0]
        assert nz.min() > 1e-30 and nz.max() < 1e30
        a.setflags(write=False)
        _SCENES[shape.name] = a
    return _SCENES[shape.name]


ZERO_BLOCK_SHAPE = "332x130"


def _widest(s, R):
    return max(s.segments or [(0, R)], key=lambda g: g[1] - g[0])


def _zero_block(x, s):
    """2w + 3 rows x 2w + 3 columns of exact zeros in the widest segment, off the zero_v_div band: the
    cells at its centre have whole windows of zeros in both stages, so their threshold is 0 and they
    pass (0 >= 0) at every rank."""
    V, R = x.shape
    n = 2 * (s.ref + s.save) + 3
    a, b = _widest(s, R)
    c0, v0 = a + (b - a - n) // 2, V - s.M0 - n - 8
    assert c0 >= a and (not s.zero_v_div or v0 >= ref.zero_v_rows(V, s.zero_v_div)[1])
    x[v0:v0 + n, c0:c0 + n] = 0.0


def _run(x, s):
    """2w + 3 equal cells of 35 in one row, nothing but the floor round them: each is alone in its
    column and a Doppler hit; the three candidates of the hit at the centre have both range windows
    inside the run, and x >= T x fails for T > 1 at every rank: the hit is dropped."""
    V, R = x.shape
    lo, hi = s.M0 + 1, V - s.M0
    w = s.ref + s.save
    n = 2 * w + 3
    a, b = _widest(s, R)
    dead = ref.zero_v_rows(V, s.zero_v_div) if s.zero_v_div else (0, 0)
    for v in range(lo + w + 1, hi - w - 1):
        if dead[0] - w - 2 <= v < dead[1] + w + 2:
            continue
        for c0 in range(a + 1, b - n):
            blk = x[v - w - 2:v + w + 3, c0 - 1:c0 + n + 1]
            if blk.max() <= 8.0 and blk.min() > 0.0:
                x[v, c0:c0 + n] = 35.0
                return
    # a crowded field: the floor is laid again round the run's place in the middle of the band
    v, c0 = (lo + hi) // 2, a + 1 + (b - a - n - 1) // 2
    blk = x[v - w - 2:v + w + 3, c0 - 1:c0 + n + 1]
    rng = np.random.default_rng(cfar_scene.SEED + V * R)
    blk[...] = np.clip(rng.rayleigh(np.sqrt(2.0 / np.pi), blk.shape), 0.05, 4.0).astype(np.float32)
    x[v, c0:c0 + n] = 35.0


def _edge_spikes(x, s):
    """A spike on the first and the last band row, and on the second and the last-but-one column, of
    every segment, each with nothing but the floor within a window's reach in its row and its column:
    the one-sided cells of both stages carry a detection at every rank of every form."""
    V, R = x.shape
    lo, hi = s.M0 + 1, V - s.M0
    w = s.ref + s.save
    dead = np.zeros(V, bool)
    if s.zero_v_div:
        a, b = ref.zero_v_rows(V, s.zero_v_div)
        dead[max(a, 0):b] = True

    def put(cells, value):
        for v, c in cells:
            row = x[v, max(c - w - 2, 0):c + w + 3]
            col = x[max(v - w - 2, 0):v + w + 3, c]
            if dead[v] or max(row.max(), col.max()) > 8.0 or min(row.min(), col.min()) == 0.0:
                continue
            x[v, c] = value
            return
        raise AssertionError("no free cell for an edge spike")

    for a, b in s.segments or [(0, R)]:
        inner = [c for c in range(a + w + 1, b - w - 1)] or list(range(a, b))
        put([(lo, c) for c in inner], 55.0)
        put([(hi - 1, c) for c in inner], 57.0)
        rows = list(range(lo + w + 1, hi - w - 1))
        put([(v, a + 1) for v in rows], 61.0)
        put([(v, b - 2) for v in rows], 63.0)


def masking_scene(seed=5, V=96, R=24, saveV=7):
    """Rayleigh noise of mean 1 below 5, and in column 11 two lines of 40 and 45, saveV + 2 rows
    apart: each lies in the other's reference window (ref 5 / guard 7).  From the rule: a window mean
    with the other line in it is at least 40 / 5 = 8, so the GO threshold T 7 is at least 56 and
    neither line passes; the 7th smallest of the ten reference cells is a noise cell below 5, so the
    union k = 7 threshold is below 35 and both pass."""
    rng = np.random.default_rng(seed)
    x = np.minimum(rng.rayleigh(np.sqrt(2.0 / np.pi), (V, R)), 4.99).astype(np.float32)
    va = V // 2
    x[va, 11] = 40.0
    x[va + saveV + 2, 11] = 45.0
    return x, (va, 11), (va + saveV + 2, 11)


MASK_PARAMS = dict(refV=5, saveV=7, refR=5, saveR=7, M0=2, TV=7.0, TR=7.0, rFlag=0)
