"""Designed CFAR scenes: a Rayleigh noise floor (mean 1, fixed seed, fp32-representable) with
named features on the cells where the CFAR kernels take another branch -- the first and last
cells of every column segment, the first and last cells with a window on either side, the rows
at the ends of the Doppler band and around the zeroed band, the column pairs that straddle the
4- and 16-cell words of the range kernels, re-localisation cases, a run that passes the Doppler
test and fails the range test, and exact zeros.

Every feature states the outcome it is there to produce (Feature.claims: cell -> (flagV, flag),
either None where nothing is claimed) from the rules of executeCFAR, not from any oracle's output;
tests/test_cfar_scene_cpu.py holds both oracles to the claims.  A feature never shares a column
within a Doppler window's reach, or a row within a range window's reach, with another one,
so a claim depends on the feature and on noise-level cells alone: a spike of 30-60 times the floor
mean against a threshold of at most T = 3 times a window mean of noise.

Features that do not fit a small field are listed in Scene.skipped (build() places the Doppler
edges first, then the range edges, then the rest); the tables in test_cfar_scene_cpu.py say which
kinds every scene must hold.

Rows are 0-based: the band is [lo, hi) = [M0 + 1, V - M0) (executeCFAR.m:23), `dead` rows are
zeroed before the CFAR (fun_0v_pressing of main_cfar.m:90, and for a scene that goes through the
MTD kernel also the MTD's own zeroed rows).  A spike on a dead row is `erased`: the scene must
give the flags of the same scene without it.
"""
from dataclasses import dataclass, field as dc_field

import numpy as np

import rsp_ref as ref

SEED = 20240923
QUIET = 0.01          # a cell that can not pass a Doppler test next to noise of mean 1


@dataclass
class Feature:
    name: str
    kind: str
    cells: list                      # (v, c, value) written into the field
    claims: dict = dc_field(default_factory=dict)   # (v, c) -> (flagV or None, flag or None), rFlag = 1
    tie: bool = False                # exact ties decide the outcome (the oracle's mask covers such cells)
    erased: bool = False             # lies on a dead row


@dataclass
class Scene:
    field: np.ndarray                # [V][R] float64, every value fp32-representable
    features: list
    skipped: list
    segments: list                   # 0-based [lo, hi), as given
    lo: int
    hi: int
    dead: np.ndarray                 # [V] bool

    def kinds(self):
        return {f.kind for f in self.features}

    def without(self, feature, floor=1.0):
        """The field with one feature's cells at the floor mean."""
        f = self.field.copy()
        for v, c, _ in feature.cells:
            f[v, c] = floor
        return f


def layout(R, w, n):
    """Column segments for a row of R cells and a range window of w = ref + guard cells.
    n = 0: none (the whole row); 1: one inner range; 3 / 4: segments given out of order with odd
    boundaries, one edge on a multiple of 16, one of exactly 2w cells, one gap of 5 cells and (4)
    one edge at 16k + 2."""
    if n == 0:
        return []
    if n == 1:
        return [(5, R - 3)]
    e1 = -(-(3 + 2 * w) // 16) * 16
    s1 = (e1, e1 + 2 * w)
    a2 = s1[1] + 5
    if n == 3:
        segs = [(3, e1), s1, (a2, R - 1)]
        order = (2, 0, 1)
    else:
        e3 = -(-(a2 + 2 * w - 2) // 16) * 16 + 2
        segs = [(3, e1), s1, (a2, e3), (e3, R - 1)]
        order = (2, 0, 3, 1)
    if any(b - a < 2 * w for a, b in segs):
        raise ValueError("%d segments of >= %d cells do not fit %d columns" % (n, 2 * w, R))
    return [segs[i] for i in order]


class _Placer:
    def __init__(self, V, R, lo, hi, dead, wv, w, rng):
        self.V, self.R, self.lo, self.hi, self.dead, self.wv, self.w, self.rng = V, R, lo, hi, dead, wv, w, rng
        self.ov = np.zeros(0, np.int64)
        self.oc = np.zeros(0, np.int64)
        self.rows = [v for v in range(lo, hi) if not dead[v]]
        self.turn = 0

    def free(self, cells):
        cv = np.array([v for v, _, _ in cells])
        cc = np.array([c for _, c, _ in cells])
        if cv.min() < 0 or cv.max() >= self.V or cc.min() < 0 or cc.max() >= self.R:
            return False
        if self.ov.size == 0:
            return True
        dv = np.abs(self.ov[:, None] - cv[None, :])
        dc = np.abs(self.oc[:, None] - cc[None, :])
        return not np.any(((dc == 0) & (dv <= self.wv + 1)) | ((dv == 0) & (dc <= self.w + 3)))

    def take(self, cells):
        self.ov = np.concatenate([self.ov, [v for v, _, _ in cells]])
        self.oc = np.concatenate([self.oc, [c for _, c, _ in cells]])

    def spike(self):
        return float(np.float32(30.0 + 30.0 * self.rng.random()))

    def row_order(self):
        """Band rows off the dead rows, starting somewhere else every time."""
        self.turn += 1
        k = (self.turn * 7) % max(len(self.rows), 1)
        return self.rows[k:] + self.rows[:k]


def build(V, R, segments, M0, zero_v_div, refV, saveV, refR, saveR, mtd_zero_div=0, seed=SEED):
    segs = [tuple(s) for s in segments] or [(0, R)]
    lo, hi = M0 + 1, V - M0
    wv, w = refV + saveV, refR + saveR
    dead = np.zeros(V, bool)
    for div in (zero_v_div, mtd_zero_div):
        if div:
            a, b = ref.zero_v_rows(V, div)
            dead[max(a, 0):b] = True
    rng = np.random.default_rng(seed)
    fld = rng.rayleigh(np.sqrt(2.0 / np.pi), (V, R)).astype(np.float32).astype(np.float64)
    P = _Placer(V, R, lo, hi, dead, wv, w, rng)
    feats, skipped = [], []
    inseg = np.zeros(R, bool)
    for a, b in segs:
        inseg[a:b] = True

    def seg_of(c):
        for a, b in segs:
            if a <= c < b:
                return a, b
        return None

    def put(f):
        P.take(f.cells)
        for v, c, x in f.cells:
            fld[v, c] = float(np.float32(x))
        feats.append(f)

    def lone(name, kind, v, c):
        """One spike at (v, c): flagged where it stands, silent off the band or the segments, erased
        on a dead row."""
        cells = [(v, c, P.spike())]
        if not P.free(cells):
            return False
        f = Feature(name, kind, cells)
        if dead[v]:
            f.erased = True
        elif not (lo <= v < hi) or not inseg[c]:
            f.claims[(v, c)] = (0, 0)
        else:
            f.claims[(v, c)] = (1, 1)
        put(f)
        return True

    def lone_any_row(name, kind, c):
        if not 0 <= c < R:
            return False
        for v in P.row_order():
            if lone(name, kind, v, c):
                return True
        skipped.append(name)
        return False

    def lone_any_col(name, kind, v):
        if not 0 <= v < V:
            return False
        a, b = max(segs, key=lambda g: g[1] - g[0])   # side by side in the widest segment, off its edge cells
        k = min(w + 2, b - a - 1)
        for c in list(range(a + k, b)) + list(range(a, a + k)):
            if lone(name, kind, v, c):
                return True
        skipped.append(name)
        return False

    # ---- Doppler edges: rows fixed, any column
    drows = [("lo-1", lo - 1), ("hi", hi), ("lo", lo), ("lo+1", lo + 1), ("lo+wv-1", lo + wv - 1), ("lo+wv", lo + wv),
             ("hi-wv-1", hi - wv - 1), ("hi-wv", hi - wv), ("hi-2", hi - 2), ("hi-1", hi - 1)]
    if zero_v_div:
        a, b = ref.zero_v_rows(V, zero_v_div)
        drows += [("zero-below", a - 1), ("zero-above", b), ("zero-inside", a)]
    seen = set()
    for nm, v in drows:
        if v in seen:
            continue
        seen.add(v)
        lone_any_col("doppler:" + nm, "doppler-edge", v)

    # ---- range edges: columns fixed, any row
    seen = set()
    for i, (a, b) in enumerate(segs):
        for nm, c in (("a", a), ("a+1", a + 1), ("a+w-1", a + w - 1), ("a+w", a + w), ("b-w-1", b - w - 1),
                      ("b-w", b - w), ("b-2", b - 2), ("b-1", b - 1)):
            if c in seen:
                continue
            seen.add(c)
            lone_any_row("seg%d:%s" % (i, nm), "range-edge", c)
    gaps = []
    cuts = sorted(segs)
    for (a0, b0), (a1, b1) in zip([(0, 0)] + cuts, cuts + [(R, R)]):
        if a1 > b0:
            gaps.append((b0, a1))
    for i, (g0, g1) in enumerate(gaps):
        lone_any_row("gap%d" % i, "range-gap", (g0 + g1) // 2)

    # ---- pairs and plateaus: values[i] at column c0 + i, quiet cells on both outer sides
    def live(v):
        """Every Doppler window of row v that fits the band has at least half its rows off the dead
        rows, so a QUIET cell of that row stays below its threshold."""
        for s in (range(v - wv, v - saveV), range(v + saveV + 1, v + wv + 1)):
            if s[0] >= lo and s[-1] < hi and 2 * sum(1 for r in s if not dead[r]) < len(s):
                return False
        return True

    def group(name, kind, c0, values, claims_of, tie=False, pillar=None):
        n = len(values)
        if c0 - 1 < 0 or c0 + n >= R:
            return False
        for v in P.row_order():
            if not live(v):
                continue
            cells = [(v, c0 - 1, QUIET)] + [(v, c0 + i, x) for i, x in enumerate(values)] + [(v, c0 + n, QUIET)]
            if pillar is not None:   # column c0 + pillar must fail its Doppler test: both windows at its value
                sides = [range(v - wv, v - saveV), range(v + saveV + 1, v + wv + 1)]
                fit = [s for s in sides if s[0] >= lo and s[-1] < hi]
                if not fit or any(dead[r] for s in fit for r in s):
                    continue
                cells += [(r, c0 + pillar, values[pillar]) for s in fit for r in s]
            if P.free(cells):
                put(Feature(name, kind, cells, claims_of(v), tie))
                return True
        return False

    def pair(name, kind, cA, cB, pillar=False):
        """A Doppler hit of value A at cA, its larger neighbour B at cB = cA +- 1: the flag moves to cB
        (same segment, guard >= 1) or each stands alone (a segment edge between them).  pillar: B's
        Doppler windows are filled with B, so B itself is no Doppler hit."""
        A, B = P.spike(), float(np.float32(70.0 + 10.0 * rng.random()))
        vals = [A, B] if cB > cA else [B, A]
        sA, sB = seg_of(cA), seg_of(cB)
        if sA is None or sB is None:
            return False

        def claims(v):
            fvB = 0 if pillar else 1
            if sA != sB:
                return {(v, cA): (1, 1), (v, cB): (fvB, fvB)}   # no hit of cB's own segment reaches it
            if saveR < 1:     # each lies in the other's reference window: no range claim
                return {(v, cA): (1, None), (v, cB): (fvB, None)}
            return {(v, cA): (1, 0), (v, cB): (fvB, 1)}
        return group(name, kind, min(cA, cB), vals, claims, pillar=(vals.index(B) if pillar else None))

    def interior(n=2, step=16):
        """Multiples c of step with c - 2 .. c + n inside one segment."""
        out = []
        for a, b in sorted(segs):
            c = -(-(a + 2) // step) * step
            while c + n < b:
                out.append(c)
                c += step
        return out

    def first(name, cands, start, fn, tries=6, record=True):
        """fn(c) on up to `tries` candidates from the start-th quarter of the list on."""
        k = (len(cands) * start) // 4
        for c in (cands[k:] + cands[:k])[:tries]:
            if fn(c):
                return True
        if record:
            skipped.append(name)
        return False

    def word(name, kind, cands, start, cols):
        """A pair across a word boundary, the larger cell no Doppler hit where its pillars fit: the
        flag then reaches it through the neighbouring word's Doppler flag alone."""
        return (first(name, cands, start, lambda c: pair(name, kind, *cols(c), pillar=True), record=False) or
                first(name, cands, start, lambda c: pair(name, kind, *cols(c))))

    c16 = interior()
    c4 = [c for c in interior(step=4) if c % 16]
    word("word16", "word-pair", c16, 1, lambda c: (c - 1, c))
    word("word16-mirror", "word-pair", c16, 2, lambda c: (c, c - 1))
    word("word4", "word-pair", c4, 1, lambda c: (c - 1, c))
    word("word4-mirror", "word-pair", c4, 3, lambda c: (c, c - 1))
    edges = sorted({a for a, _ in segs} | {b for _, b in segs})
    for nm, off in (("edge16", 0), ("edge16+2", 2)):
        ks = [e - off for e in edges if (e - off) % 16 == 0 and e - off > 0 and seg_of(e - off - 1) and seg_of(e - off)]
        word(nm, "word-edge", ks, 0, lambda k: (k - 1, k))

    # ---- re-localisation
    cs = [c for c in interior(n=3, step=1) if c % 4 == 1]
    first("reloc-moved", cs, 2, lambda c: pair("reloc-moved", "reloc", c, c + 1, pillar=True))

    def equal(c):
        x = P.spike()
        ok = saveR >= 1   # else each lies in the other's reference window
        return group("reloc-equal", "reloc-tie", c, [x, x],
                     lambda v: {(v, c): (1, 1 if ok else None), (v, c + 1): (1, 0 if ok else None)}, tie=True)

    def plateau(c):
        x = P.spike()
        ok = saveR >= 2
        return group("reloc-plateau", "reloc-tie", c, [x, x, x],
                     lambda v: {(v, c): (1, 1 if ok else None), (v, c + 1): (1, 1 if ok else None),
                                (v, c + 2): (1, 0 if ok else None)}, tie=True)

    def boundary(b):
        x = P.spike()
        return group("reloc-boundary", "reloc-boundary", b - 1, [x, x], lambda v: {(v, b - 1): (1, 1), (v, b): (1, 1)})

    first("reloc-equal", cs, 1, equal)
    first("reloc-plateau", cs, 3, plateau)
    first("reloc-boundary", [b for a, b in sorted(segs) if seg_of(b) is not None], 0, boundary)

    # ---- Doppler yes, range no: 2w + 8 equal cells in one row; the 8 centre cells have both windows
    # inside the run (x >= T x fails for T > 1), and a cell that fails is never flagged
    def run(c0):
        x = P.spike()
        return group("run", "run", c0, [x] * (2 * w + 8), lambda v: {(v, c0 + w + i): (1, 0) for i in range(8)},
                     tie=True)

    big = sorted(segs, key=lambda s: s[0] - s[1])
    first("run", [c for a, b in big for c in range(a + 1, b - 2 * w - 8, 4)], 0, run, tries=1 << 30)

    # ---- exact zeros: every row of 2w + 6 columns; the Doppler test is 0 >= T * 0 on every band cell,
    # the range test likewise on the 6 centre columns, and the first of three equal candidates wins
    # (claimed where the hit one column up has all three of its candidates inside the block)
    def zeros(c0):
        n = 2 * w + 6
        if np.any((P.oc > c0 - w - 4) & (P.oc < c0 + n + w + 3)):
            return False
        cells = [(v, c0 + i, 0.0) for v in range(V) for i in range(n)]
        claims = {(v, c0 + i): (1, 1 if w <= i < min(w + 6, 2 * w + 4) else None) for v in range(lo, hi) for i in range(n)}
        put(Feature("zeros", "zeros", cells, claims))
        return True

    def zeros_small(c0):   # no room for that: a small block, nothing claimed of it
        for v in P.row_order():
            cells = [(v + dv, c0 + i, 0.0) for dv in range(2) for i in range(3)]
            if v + 1 < hi and P.free(cells):
                put(Feature("zeros-small", "zeros-small", cells))
                return True
        return False

    if not first("zeros", [c for a, b in big for c in range(a, b - 2 * w - 5, 3)], 0, zeros, tries=1 << 30):
        skipped.remove("zeros")
        first("zeros-small", list(range(2, R - 4, 5)), 1, zeros_small, tries=1 << 30)
    return Scene(fld, feats, skipped, [tuple(s) for s in segments], lo, hi, dead)


def claimed(scene, rflag=1):
    """[(feature, (v, c), flagV or None, flag or None)] of the features off the dead rows; with
    rFlag = 0 the flag is the Doppler flag."""
    out = []
    for f in scene.features:
        for cell, (fv, fl) in f.claims.items():
            out.append((f, cell, fv, fl if rflag else fv))
    return out


def to_pc(field, window, rng):
    """Pulse-compressed rows [P][R] complex64 whose windowed, fftshifted slow-time FFT has the
    field's magnitudes: random phases, inverse shift, inverse transform per column in fp64, divided
    by the slow-time window."""
    V = field.shape[0]
    ph = np.exp(2j * np.pi * rng.random(field.shape))
    X = np.fft.ifftshift(field * ph, axes=0)
    x = np.fft.ifft(X, axis=0) / np.asarray(window, np.float64)[:, None]
    assert x.shape[0] == V
    return x.astype(np.complex64)
