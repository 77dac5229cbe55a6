"""Stacked-beam fusion on the GPU (rsp_beam_fuse_dev / rsp_beam_elev_dev, csrc/rsp_fuse.hip) against the
restatement tests/fuse_ref.py, through the C ABI itself so that the bases, the pitch, the strides and every
output buffer are the test's own; the last tests go through rsp.fuse on Engine.window_dev's planes.

The fuse kernel makes the same float32 compares in the same order: all four outputs are compared byte for
byte, with sentinel bytes round every output.  The elevation is byte for byte under laws 0 and 1.  Under
law 2 the device's log and the host's may each be one ulp off, so every branch decision (d_hb) is exact and
el is held within a bound the test computes per hit from the restatement: the largest change of el when
each of the three logarithms moves by -2, 0 or +2 ulp (27 combinations), plus 4 ulp of |el|.
"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import fuse_ref as fr

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel bytes (a multiple of 4) on each side of every output
SENT = 0xA5
DEV = "cuda:0"

# (V, R, ld, column offset of the window, elements the input and output buffers are moved off their
# allocation's alignment)
SHAPES = [(5, 1, 1, 0, 0), (5, 7, 7, 0, 0), (64, 67, 67, 0, 0), (33, 130, 133, 3, 1), (16, 512, 574, 62, 0)]
SHAPE_IDS = ["5x1", "5x7", "64x67", "33x130of133odd", "16x512of574at62"]
X13 = np.cumsum([0.0, 2.1, 1.8, 2.3, 1.9, 2.0, 2.4, 1.7, 2.2, 1.95, 2.05, 1.85, 2.15]) - 3.0


def _centres(K):
    return X13.copy() if K == 13 else 1.5 * np.arange(K) - 4.0


@pytest.fixture(scope="module")
def rt():
    import torch
    from rsp import _capi as capi
    lib = capi.load_library()
    ctx = C.c_void_p()
    capi.check(lib.rsp_create(C.byref(ctx), 0, None), None)   # the CFAR-only kind
    yield capi, lib, ctx
    torch.cuda.synchronize()
    lib.rsp_destroy(ctx)


def _scene(seed, B, K, V, ld):
    """Full-pitch planes [B][K][V][ld]: noise magnitudes with exact ties between beams planted in them, and
    sparse flags with some bytes other than 1; a few cells are flagged in every beam."""
    rng = np.random.default_rng(seed)
    amp = np.abs(rng.standard_normal((B, K, V, ld))).astype(np.float32)
    for _ in range(2 * K):
        k1, k2 = rng.integers(0, K, 2)
        tie = rng.random((B, V, ld)) < 0.15
        amp[:, k2][tie] = amp[:, k1][tie]
    flag = (rng.random((B, K, V, ld)) < min(0.12, 0.5 / K)).astype(np.uint8)      # about 4 cells in 10 hit in some beam
    flag *= rng.integers(1, 256, size=flag.shape, dtype=np.uint8)
    full = np.broadcast_to((rng.random((B, V, ld)) < 0.03)[:, None], flag.shape)
    flag[full & (flag == 0)] = 1
    return amp, flag


def _params(capi, K, min_beams, law, ld, bs, cs, beam_el=None):
    p = capi.rsp_fuse_params()
    p.beams, p.min_beams, p.law, p.reserved = K, min_beams, law, 0
    p.ld, p.beam_stride, p.cpi_stride = ld, bs, cs
    for k, x in enumerate(_centres(K) if beam_el is None else beam_el):
        p.beam_el[k] = float(x)
    return p


class Planes:
    """The input planes on the device in one of the two layouts, `off` elements off their allocation."""

    def __init__(self, amp, flag, layout, off=0):
        import torch
        self.B, self.K, self.V, self.ld = amp.shape
        B, K, V, ld = amp.shape
        if layout == "cpi":       # [batch][beams][V][ld]
            a, f = amp, flag
            self.bs, self.cs = V * ld, K * V * ld
        else:                     # [beams][batch][V][ld], as rsp_window_pc_mtd_cfar_dev writes
            a, f = amp.transpose(1, 0, 2, 3), flag.transpose(1, 0, 2, 3)
            self.bs, self.cs = B * V * ld, V * ld
        n = B * K * V * ld
        self.d_amp = torch.zeros(n + off, dtype=torch.float32, device=DEV)
        self.d_amp[off:].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        self.d_flag = torch.zeros(n + off, dtype=torch.uint8, device=DEV)
        self.d_flag[off:].copy_(torch.from_numpy(np.ascontiguousarray(f).reshape(-1)))
        self.off = off

    def amp_ptr(self, b0=0, col0=0):
        return self.d_amp.data_ptr() + 4 * (self.off + b0 * self.cs + col0)

    def flag_ptr(self, b0=0, col0=0):
        return self.d_flag.data_ptr() + self.off + b0 * self.cs + col0


def _gpu_fuse(rt, pl, R, col0, min_beams, famp=True, fcnt=True, cuts=None, out_off=None):
    """rsp_beam_fuse_dev on the window col0 .. col0+R-1, as one call or as the calls `cuts` names; returns the
    four outputs as numpy (None where not asked for) after checking every sentinel."""
    import torch
    capi, lib, ctx = rt
    B, V, K = pl.B, pl.V, pl.K
    n = B * V * R
    off = pl.off if out_off is None else out_off
    bufs = {}
    for name, esz in (("fflag", 1), ("fbeam", 1), ("famp", 4), ("fcnt", 1)):
        bufs[name] = torch.empty(2 * GUARD + (n + off) * esz, dtype=torch.uint8, device=DEV).fill_(SENT)
    want = dict(fflag=True, fbeam=True, famp=famp, fcnt=fcnt)
    p = _params(capi, K, min_beams, 2, pl.ld, pl.bs, pl.cs)
    st = torch.cuda.current_stream().cuda_stream
    cuts = cuts or [0, B]
    for a, b in zip(cuts[:-1], cuts[1:]):
        ptr = lambda name, esz: bufs[name].data_ptr() + GUARD + (off + a * V * R) * esz if want[name] else None   # noqa: E731
        capi.check(lib.rsp_beam_fuse_dev(ctx, pl.amp_ptr(a, col0), pl.flag_ptr(a, col0), V, R, b - a, C.byref(p),
                                         ptr("fflag", 1), ptr("fbeam", 1), ptr("famp", 4), ptr("fcnt", 1), C.c_void_p(st)), ctx)
    torch.cuda.synchronize()
    out = []
    for name, esz, dt in (("fflag", 1, np.uint8), ("fbeam", 1, np.uint8), ("famp", 4, np.float32), ("fcnt", 1, np.uint8)):
        raw = bufs[name].cpu().numpy()
        lead = GUARD + off * esz
        if not want[name]:
            assert (raw == SENT).all(), "%s was written though it was not asked for" % name
            out.append(None)
            continue
        assert (raw[:lead] == SENT).all() and (raw[lead + n * esz:] == SENT).all(), "%s's guards were written" % name
        out.append(raw[lead:lead + n * esz].copy().view(dt).reshape(B, V, R))
    return out


def _same(got, want, what):
    for name, g, w in zip(("fflag", "fbeam", "famp", "fcnt"), got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            iv = {4: np.uint32, 1: np.uint8}[g.dtype.itemsize]
            bad = np.argwhere(g.view(iv) != w.view(iv))
            raise AssertionError("%s: %s differs at %d places, first %s: got %r, want %r"
                                 % (what, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


_SCENES = {}


def _shared(K, shape):
    """One scene and its restatement per (beams, shape), shared by the tests that need it and left unchanged."""
    key = (K, shape)
    if key not in _SCENES:
        V, R, ld, col0, off = shape
        amp, flag = _scene(100 * K + V + R, 3, K, V, ld)
        a, f = np.ascontiguousarray(amp[..., col0:col0 + R]), np.ascontiguousarray(flag[..., col0:col0 + R])
        _SCENES[key] = (amp, flag, {m: fr.fuse(a, f, m) for m in sorted({1, 2, K})})
    return _SCENES[key]


# ---------------------------------------------------------------- fuse against the restatement
@pytest.mark.parametrize("layout", ["cpi", "beam"])
@pytest.mark.parametrize("K", [2, 3, 13, 32])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fuse_matches_the_restatement(rt, shape, K, layout):
    V, R, ld, col0, off = shape
    amp, flag, want = _shared(K, shape)
    pl = Planes(amp, flag, layout, off)
    for i, m in enumerate(sorted(want)):
        w = want[m]
        assert 0 < w[0].sum() < w[0].size or R * V < 40, "the scene flags nothing or everything"
        _same(_gpu_fuse(rt, pl, R, col0, m), w, "min_beams %d" % m)
        if i == 0:      # the nullable outputs: each alone, then neither
            _same(_gpu_fuse(rt, pl, R, col0, m, famp=False), w, "no d_famp")
            _same(_gpu_fuse(rt, pl, R, col0, m, fcnt=False), w, "no d_fcnt")
            _same(_gpu_fuse(rt, pl, R, col0, m, famp=False, fcnt=False), w, "neither")


def test_the_scenes_hold_what_they_are_for():
    """Conditions on the inputs: ties between the flagged beams of a cell where the first must win, flag bytes
    other than 1, cells where min_beams = beams passes, hits whose peak beam is weaker than famp."""
    amp, flag, want = _shared(13, SHAPES[3])
    V, R, ld, col0, off = SHAPES[3]
    a, f = amp[..., col0:col0 + R], flag[..., col0:col0 + R]
    fflag, fbeam, famp, fcnt = want[1]
    hit = fflag == 1
    masked = np.where(f != 0, a, -1.0)
    top = masked.max(axis=1)
    assert (((masked == top[:, None]) & (f != 0)).sum(axis=1)[hit] > 1).sum() > 20        # tied flagged maxima
    assert (f > 1).sum() > 100 and want[13][0].sum() > 5 and (want[2][0].sum() < want[1][0].sum())
    assert (np.take_along_axis(a, np.where(hit, fbeam, 0)[:, None].astype(np.int64), axis=1)[:, 0][hit] < famp[hit]).sum() > 100


# ---------------------------------------------------------------- vector path against the cell-by-cell path
@pytest.mark.parametrize("layout", ["cpi", "beam"])
@pytest.mark.parametrize("V,R,ld,col0", [(16, 512, 574, 62), (9, 64, 64, 0), (7, 130, 132, 0)], ids=["long", "64", "130of132"])
def test_vector_path_equals_the_cell_path(rt, layout, V, R, ld, col0):
    """Aligned, every thread whose four cells fit takes the 16-byte / 4-byte loads and stores; moved off by one
    element (inputs, outputs, or both) every thread takes its cells one by one.  Same bytes."""
    amp, flag = _scene(7 + R, 2, 13, V, ld)
    want = fr.fuse(amp[..., col0:col0 + R], flag[..., col0:col0 + R], 2)
    for in_off, out_off in ((0, 0), (1, 1), (1, 0), (0, 1), (2, 2), (4, 4)):
        pl = Planes(amp, flag, layout, in_off)
        _same(_gpu_fuse(rt, pl, R, col0, 2, out_off=out_off), want, "inputs off by %d, outputs by %d" % (in_off, out_off))


# ---------------------------------------------------------------- split invariance
@pytest.mark.parametrize("layout", ["cpi", "beam"])
def test_a_batch_equals_its_cpis_one_by_one(rt, layout):
    V, R, ld, col0, off = SHAPES[3]
    amp, flag = _scene(31, 4, 13, V, ld)
    pl = Planes(amp, flag, layout, 0)
    whole = _gpu_fuse(rt, pl, R, col0, 2)
    _same(_gpu_fuse(rt, pl, R, col0, 2, cuts=[0, 1, 2, 3, 4]), whole, "one by one")
    _same(_gpu_fuse(rt, pl, R, col0, 2, cuts=[0, 3, 4]), whole, "3 + 1")
    _same(_gpu_fuse(rt, pl, R, col0, 2), whole, "run to run")
    _same(whole, fr.fuse(amp[..., col0:col0 + R], flag[..., col0:col0 + R], 2), "restatement")


# ---------------------------------------------------------------- elevation
def _elev_scene(seed, B, K, V, R, x):
    """Noise planes with designed triples at flagged cells: Gaussian-beam triples (|den| well away from zero),
    and the degenerate ones whose branch does not hang on an ulp of a logarithm: equal amplitudes (flat: the
    same input gives the same logarithm, den = 0 exactly), a peak beam weaker than both unflagged neighbours
    (convex), zero and negative neighbours, an edge peak beam, a strongly one-sided triple (the clamp)."""
    rng = np.random.default_rng(seed)
    amp = (0.05 * np.abs(rng.standard_normal((B, K, V, R)))).astype(np.float32)
    flag = np.zeros((B, K, V, R), np.uint8)
    kinds = ["gauss", "flat", "convex", "zero", "negative", "edge_lo", "edge_hi", "clamp", "pair"]
    n = 0
    for b in range(B):
        for v in range(3, V - 3, 2):
            for r in range(3 + (v % 4), R - 3, 5):
                kind = kinds[n % len(kinds)]
                n += 1
                k = int(rng.integers(1, K - 1))
                if kind == "gauss" or kind == "pair":
                    t = rng.uniform(0.5 * (x[k - 1] + x[k]), 0.5 * (x[k] + x[k + 1]))
                    w = rng.uniform(3.0, 6.0)
                    amp[b, :, v, r] = (50.0 * np.exp(-4.0 * math.log(2.0) * (t - x) ** 2 / w ** 2)).astype(np.float32)
                    flag[b, k, v, r] = 3
                    if kind == "pair":
                        flag[b, k - 1, v, r] = 1
                        flag[b, k + 1, v, r] = 1
                elif kind == "flat":
                    amp[b, k - 1:k + 2, v, r] = 7.0
                    flag[b, k, v, r] = 1
                elif kind == "convex":
                    amp[b, k - 1:k + 2, v, r] = (9.0, 2.0, 8.0)
                    flag[b, k, v, r] = 1
                elif kind == "zero":
                    amp[b, k - 1:k + 2, v, r] = (0.0, 5.0, 3.0)
                    flag[b, k, v, r] = 1
                elif kind == "negative":
                    amp[b, k - 1:k + 2, v, r] = (2.0, 5.0, -3.0)
                    flag[b, k, v, r] = 1
                elif kind == "edge_lo":
                    amp[b, 0:2, v, r] = (6.0, 5.0)
                    flag[b, 0, v, r] = 1
                elif kind == "edge_hi":
                    amp[b, K - 2:K, v, r] = (5.0, 6.0)
                    flag[b, K - 1, v, r] = 1
                else:
                    amp[b, k - 1:k + 2, v, r] = (0.01, 1.0, 20.0)     # unflagged stronger neighbour: beyond the clamp
                    flag[b, k, v, r] = 1
    return amp, flag


class _MovedLog:
    """math.log with the next three results moved by the given numbers of ulp."""

    def __init__(self, moves):
        self.moves = list(moves)

    def __call__(self, a):
        y = math.log(a)
        return y + self.moves.pop(0) * math.ulp(y)


def _law2_bound(k, x, am, a0, ap, e):
    worst = 0.0
    for mv in itertools.product((-2, 0, 2), repeat=3):
        e2, _ = fr.elev_one(2, k, x, am, a0, ap, log=_MovedLog(mv))
        worst = max(worst, abs(e2 - e))
    return worst + 4 * math.ulp(abs(e))


def _measure(rt, famp, fflag, B, V, R, max_hits):
    """The hit lists rsp_motion_measure_dev makes on d_famp / d_fflag: est prefilled with a sentinel."""
    import torch
    capi, lib, ctx = rt
    mp = capi.rsp_measure_params()
    mp.extra_dots, mp.r_interp, mp.v_interp, mp.mtd0_num, mp.beam_pos_num = 2, 8, 4, 0, 0
    mp.delta_r, mp.delta_v, mp.k_value, mp.beam_angle_step, mp.ele_comp, mp.ele_sys_err = 12.0, 0.5, 10.0, 5.0, 0.0, 0.0
    mp.ld, mp.cpi_stride = R, V * R
    d_famp = torch.from_numpy(famp).to(DEV)
    d_fflag = torch.from_numpy(fflag).to(DEV)
    rs = torch.arange(R, dtype=torch.float64, device=DEV) * 12.0
    vs = torch.arange(V, dtype=torch.float64, device=DEV) * 0.5
    est = torch.full((B, max_hits, 3), -777.0, dtype=torch.float64, device=DEV)
    cells = torch.full((B, max_hits, 2), -5, dtype=torch.int32, device=DEV)
    count = torch.zeros((B, 2), dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    capi.check(lib.rsp_motion_measure_dev(ctx, d_famp.data_ptr(), d_famp.data_ptr(), d_fflag.data_ptr(), V, R, B, C.byref(mp),
                                          rs.data_ptr(), vs.data_ptr(), max_hits, est.data_ptr(), cells.data_ptr(),
                                          count.data_ptr(), C.c_void_p(st)), ctx)
    torch.cuda.synchronize()
    return est, cells, count


@pytest.fixture(scope="module")
def elev_case(rt):
    """One designed scene, fused on the device, and its measured hit lists; shared and left unchanged."""
    B, K, V, R = 2, 13, 33, 130
    x = _centres(K)
    amp, flag = _elev_scene(5, B, K, V, R, x)
    pl = Planes(amp, flag, "beam", 0)
    fflag, fbeam, famp, fcnt = _gpu_fuse(rt, pl, R, 0, 1)
    _same((fflag, fbeam, famp, fcnt), fr.fuse(amp, flag, 1), "the designed scene")
    return dict(B=B, K=K, V=V, R=R, x=x, amp=amp, flag=flag, pl=pl, fflag=fflag, fbeam=fbeam, famp=famp)


def _gpu_elev(rt, c, law, max_hits, hb=True, x=None, stride3=True):
    import torch
    capi, lib, ctx = rt
    B, K, V, R, pl = c["B"], c["K"], c["V"], c["R"], c["pl"]
    est, cells, count = _measure(rt, c["famp"], c["fflag"], B, V, R, max_hits)
    before = est.cpu().numpy().copy()
    d_fbeam = torch.from_numpy(c["fbeam"]).to(DEV)
    d_hb = torch.full((B, max_hits, 4), -9, dtype=torch.int32, device=DEV)
    dense = torch.full((B, max_hits), -777.0, dtype=torch.float64, device=DEV)
    p = _params(capi, K, 1, law, pl.ld, pl.bs, pl.cs, beam_el=c["x"] if x is None else x)
    st = torch.cuda.current_stream().cuda_stream
    capi.check(lib.rsp_beam_elev_dev(ctx, pl.amp_ptr(), pl.flag_ptr(), d_fbeam.data_ptr(), V, R, B, C.byref(p),
                                     cells.data_ptr(), count.data_ptr(), max_hits,
                                     est.data_ptr() + 16 if stride3 else dense.data_ptr(), 3 if stride3 else 1,
                                     d_hb.data_ptr() if hb else None, C.c_void_p(st)), ctx)
    torch.cuda.synchronize()
    after = est.cpu().numpy()
    cn, cl = count.cpu().numpy(), cells.cpu().numpy()
    if stride3:
        # the neighbours est[..][0..1] and every slot past the count keep their bytes
        assert after[:, :, :2].tobytes() == before[:, :, :2].tobytes()
        el = after[:, :, 2].copy()
        assert dense.cpu().numpy().tobytes() == np.full((B, max_hits), -777.0).tobytes()
    else:
        assert after.tobytes() == before.tobytes()
        el = dense.cpu().numpy()
    for b in range(B):
        n = min(int(cn[b, 0]), max_hits)
        assert (el[b, n:] == -777.0).all(), "slots past the count were written"
    hbn = d_hb.cpu().numpy()
    if not hb:
        assert (hbn == -9).all()
    return el, hbn, cl, cn


@pytest.mark.parametrize("max_hits", [400, 17, 0], ids=["all", "17", "none"])
@pytest.mark.parametrize("law", [0, 1])
def test_elevation_laws_0_and_1_byte_for_byte(rt, elev_case, law, max_hits):
    c = elev_case
    el, hb, cells, count = _gpu_elev(rt, c, law, max_hits)
    assert (count[:, 0] > 100).all() and (count[:, 0] < 400).all(), count
    want_el, want_hb = fr.elevation(c["amp"], c["flag"], c["fbeam"], cells, count, c["x"], law)
    for b in range(c["B"]):
        n = min(int(count[b, 0]), max_hits)
        assert el[b, :n].tobytes() == want_el[b, :n].tobytes(), (law, b)
        assert hb[b, :n].tobytes() == want_hb[b, :n].tobytes(), (law, b)
        assert (hb[b, n:] == -9).all()
    if law == 1 and max_hits == 400:
        assert (want_hb[..., 2] >= 0).sum() > 100 and ((want_hb[..., 0] >= 0) & (want_hb[..., 2] < 0)).sum() > 20


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_elevation_law_2_branches_exact_value_within_the_log_bound(rt, elev_case, descending):
    c = elev_case
    x = -c["x"] if descending else c["x"]
    el, hb, cells, count = _gpu_elev(rt, c, 2, 400, x=x)
    want_el, want_hb = fr.elevation(c["amp"], c["flag"], c["fbeam"], cells, count, x, 2)
    three = clamped = worst = 0
    for b in range(c["B"]):
        n = int(count[b, 0])
        assert hb[b, :n].tobytes() == want_hb[b, :n].tobytes(), b          # every branch decision
        for i in range(n):
            k, cnt, am, a0, ap = fr.hit_inputs(c["amp"], c["flag"], c["fbeam"], b, int(cells[b, i, 0]), int(cells[b, i, 1]), c["K"])
            e = want_el[b, i]
            if want_hb[b, i, 2] < 0:
                assert el[b, i] == e, (b, i, k)                             # x_k itself: exact
                continue
            three += 1
            clamped += e in (x[k - 1], x[k + 1])
            bound = _law2_bound(k, x, am, a0, ap, e)
            assert bound < 1e-9, (b, i, k, am, a0, ap, bound)               # the designed triples keep it small
            assert abs(el[b, i] - e) <= bound, (b, i, k, el[b, i], e, bound)
            worst = max(worst, abs(el[b, i] - e) / bound)
    print("law 2: %d three-beam hits (%d clamped), worst |el - ref| / bound = %.3g" % (three, clamped, worst))
    assert three > 60 and clamped > 10


def test_elevation_dense_output_and_no_hb(rt, elev_case):
    c = elev_case
    el, hb, cells, count = _gpu_elev(rt, c, 1, 400, hb=False, stride3=False)
    want_el, _ = fr.elevation(c["amp"], c["flag"], c["fbeam"], cells, count, c["x"], 1)
    for b in range(c["B"]):
        n = int(count[b, 0])
        assert el[b, :n].tobytes() == want_el[b, :n].tobytes()


def test_elevation_reads_a_stale_or_foreign_hit_list_safely(rt, elev_case):
    """Cells outside the planes, cells without a fused hit and a beam number that does not exist give NaN
    and {-1, cnt, -1, -1}; nothing outside the listed slots is written."""
    import torch
    capi, lib, ctx = rt
    c = elev_case
    B, K, V, R, pl = c["B"], c["K"], c["V"], c["R"], c["pl"]
    fbeam = c["fbeam"].copy()
    fbeam[0, 5, 7] = 200                                   # no such beam
    cells = np.array([[[5, 7], [-1, 0], [0, R], [V, 0], [0, 0], [2 ** 31 - 1, -2 ** 31]]] * B, np.int32)
    count = np.array([[5, 0], [-3, 0]], np.int32)
    d_cells, d_count = torch.from_numpy(cells).to(DEV), torch.from_numpy(count).to(DEV)
    d_el = torch.full((B, 6), -777.0, dtype=torch.float64, device=DEV)
    d_hb = torch.full((B, 6, 4), -9, dtype=torch.int32, device=DEV)
    d_fbeam = torch.from_numpy(fbeam).to(DEV)
    p = _params(capi, K, 1, 2, pl.ld, pl.bs, pl.cs, beam_el=c["x"])
    capi.check(lib.rsp_beam_elev_dev(ctx, pl.amp_ptr(), pl.flag_ptr(), d_fbeam.data_ptr(), V, R, B, C.byref(p), d_cells.data_ptr(),
                                     d_count.data_ptr(), 6, d_el.data_ptr(), 1, d_hb.data_ptr(),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), ctx)
    torch.cuda.synchronize()
    el, hb = d_el.cpu().numpy(), d_hb.cpu().numpy()
    want_el, want_hb = fr.elevation(c["amp"], c["flag"], fbeam, cells, count, c["x"], 2)
    assert np.isnan(el[0, :5]).all() and el[0, 5] == -777.0 and (el[1] == -777.0).all()
    assert hb[0, :5].tobytes() == want_hb[0, :5].tobytes() and (hb[0, 5] == -9).all() and (hb[1] == -9).all()
    assert hb[0, 0].tolist() == [-1, int((c["flag"][0, :, 5, 7] != 0).sum()), -1, -1]


# ---------------------------------------------------------------- the v2 stream through rsp.fuse
@pytest.fixture(scope="module")
def v2():
    """Engine.window_dev on 13 beams of synthetic echo: the planes the v2 capture hands to the fusion."""
    import torch
    from rsp import presets, synth
    from rsp.engine import Engine
    P, R, beams, nf, win = 64, 1024, 13, 1, 2
    spec = presets.v2(P, R)
    eng = Engine(spec, device=0)
    frames = synth.echo_numpy(spec, beams * (nf + 1), seed=77).reshape(beams, nf + 1, P, R)
    shp = (beams, nf, win, P, spec.R_out)
    rdm = torch.empty(shp, dtype=torch.float32, device=DEV)
    flag = torch.empty(shp, dtype=torch.uint8, device=DEV)
    eng.window_dev(torch.from_numpy(frames).to(DEV), win, rdm=rdm, flag=flag, cfar=presets.default_cfar(spec))
    torch.cuda.synchronize()
    yield eng, rdm, flag
    eng.close()


def test_window_dev_planes_fuse_without_a_copy(v2):
    import torch
    from rsp.fuse import BeamFuser
    eng, rdm, flag = v2
    amp, flg = rdm.flatten(1, 2).transpose(0, 1), flag.flatten(1, 2).transpose(0, 1)
    assert amp.data_ptr() == rdm.data_ptr() and flg.data_ptr() == flag.data_ptr() and not amp.is_contiguous()
    fuser = BeamFuser(X13, min_beams=1, engine=eng)
    got = [t.cpu().numpy() for t in fuser.fuse_dev(amp, flg)]
    _same(got, fr.fuse(amp.cpu().numpy(), flg.cpu().numpy(), 1), "window_dev's planes")
    assert 0 < got[0].sum() < got[0].size
    # the contiguous [batch][beams][V][R] copy gives the same bytes; other layouts are refused, not copied
    _same([t.cpu().numpy() for t in fuser.fuse_dev(amp.contiguous(), flg.contiguous())], got, "the contiguous copy")
    with pytest.raises(ValueError, match="one layout"):
        fuser.fuse_dev(amp, flg.contiguous())
    with pytest.raises(ValueError, match="adjacent"):
        fuser.fuse_dev(amp.transpose(2, 3), flg.transpose(2, 3))
    with pytest.raises(ValueError, match="float32"):
        fuser.fuse_dev(amp.double(), flg)
    from rsp._capi import RspError
    with pytest.raises(RspError, match="overlap"):      # CPIs one element apart: refused before anything runs
        fuser.fuse_dev(amp.as_strided(amp.shape, (1, amp.stride(1), amp.stride(2), 1)),
                       flg.as_strided(flg.shape, (1, flg.stride(1), flg.stride(2), 1)))
    fuser.close()


def test_a_stacked_beam_scene_becomes_plots_with_elevation(v2):
    """Two targets injected into the 13 planes with Gaussian beam weights: one fused hit per target cell, the
    right peak beam, law 2's elevation within the CPU test's 1e-5 deg of truth, and plots_dev equal to the
    composition by hand, byte for byte."""
    import torch
    from rsp.condense import Condense
    from rsp.fuse import BeamFuser
    from rsp.measure import Measure
    eng, rdm0, _ = v2
    rdm = rdm0.clone()
    flag = torch.zeros(rdm.shape, dtype=torch.uint8, device=DEV)
    beams, nf, win, V, R = rdm.shape
    top = float(rdm.max().item())
    targets = [dict(v=20, r=300, el=float(X13[4]) + 0.61, w=4.5), dict(v=41, r=700, el=float(X13[6]) - 0.37, w=4.5)]
    for t in targets:
        wgt = np.exp(-4.0 * math.log(2.0) * (t["el"] - X13) ** 2 / t["w"] ** 2)
        a = torch.from_numpy((100.0 * top * wgt).astype(np.float32)).to(DEV)
        rdm[:, :, :, t["v"], t["r"]] = a[:, None, None]
        flag[:, :, :, t["v"], t["r"]] = torch.from_numpy((wgt > 0.3).astype(np.uint8)).to(DEV)[:, None, None]
        t["k"] = int(np.argmax(wgt))
    assert [t["k"] for t in targets] == [4, 6]
    amp, flg = rdm.flatten(1, 2).transpose(0, 1), flag.flatten(1, 2).transpose(0, 1)
    assert amp.data_ptr() == rdm.data_ptr()
    B = nf * win
    fuser = BeamFuser(X13, min_beams=2, law="logparab", engine=eng)
    meas, cond = Measure(device=0), Condense(device=0)
    params = Measure.params(2, 12.0, 8, 0.5, 4, 10.0, 0, 5.0, 0.0, 0.0, 2)
    rs, vs = np.arange(R) * 12.0, np.arange(V) * 0.5
    fflag, fbeam, famp, fcnt = fuser.fuse_dev(amp, flg)
    assert int(fflag.sum().item()) == 2 * B                        # one fused hit per target cell
    for t in targets:
        assert (fflag[:, t["v"], t["r"]] == 1).all() and (fbeam[:, t["v"], t["r"]] == t["k"]).all()
        assert (fcnt[:, t["v"], t["r"]] >= 2).all()
    for condense in (None, cond, (cond, dict(gap=(1, 1), max_plots=64))):
        est, cells, count = fuser.plots_dev(amp, flg, (meas, params), rs, vs, condense=condense, max_hits=64)
        # by hand
        hits = fflag
        if condense is not None:
            kw = condense[1] if isinstance(condense, tuple) else {}
            hits = cond.condense_dev(famp, fflag, **kw)[0]
        est2, cells2, count2 = meas.measure_dev(famp, famp, hits, params, rs, vs, max_hits=64)
        hb = torch.full((B, 64, 4), -9, dtype=torch.int32, device=DEV)
        fuser.elevation_dev(amp, flg, fbeam, cells2, count2, est=est2, hb=hb)
        dense = fuser.elevation_dev(amp, flg, fbeam, cells2, count2)
        torch.cuda.synchronize()
        assert count.cpu().numpy().tobytes() == count2.cpu().numpy().tobytes()
        assert count.cpu().numpy()[:, 0].tolist() == [2] * B and not count.cpu().numpy()[:, 1].any()
        e, e2, cl = est.cpu().numpy(), est2.cpu().numpy(), cells.cpu().numpy()
        assert e[:, :2].tobytes() == e2[:, :2].tobytes() and cl[:, :2].tobytes() == cells2.cpu().numpy()[:, :2].tobytes()
        assert dense.cpu().numpy()[:, :2].tobytes() == e[:, :2, 2].tobytes() and np.isnan(dense.cpu().numpy()[:, 2:]).all()
        for b in range(B):
            for i in range(2):
                t = [t for t in targets if (t["v"], t["r"]) == tuple(cl[b, i])][0]
                assert abs(e[b, i, 2] - t["el"]) < 1e-5, (b, i, e[b, i, 2], t["el"])
                assert hb.cpu().numpy()[b, i].tolist() == [t["k"], int(fcnt[b, t["v"], t["r"]].item()), t["k"] - 1, t["k"] + 1]
    # and on to the tracker, unchanged
    from rsp.track import Tracker
    trk = Tracker(device=0, dt=0.08, gate=(50.0, 5.0), confirm=(1, 1))
    assign, _, _, tcount = trk.update_dev(est, count)
    torch.cuda.synchronize()
    assert (assign.cpu().numpy()[:, :2] > 0).all() and tcount.cpu().numpy()[-1, 0] == 2
    for o in (trk, meas, cond, fuser):
        o.close()
