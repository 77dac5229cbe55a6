"""Stacked-beam fusion, CPU side: the restatement tests/fuse_ref.py against hand-worked cases, law 2 on
noise-free Gaussian beams against the true elevation, the C ABI's refusals (rsp_beam_fuse_dev /
rsp_beam_elev_dev check everything they can before they look at the context), the ctypes struct against
the header, and the kernel's elevation header (csrc/rsp_fuse_math.h) compiled for the host, plain and with
the address / undefined-behaviour sanitizers, against the restatement bit for bit.
"""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import fuse_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cell(amps, flags, min_beams):
    """One cell: (fflag, fbeam, famp, fcnt) as Python numbers."""
    a = np.array(amps, np.float32).reshape(1, -1, 1, 1)
    f = np.array(flags, np.uint8).reshape(1, -1, 1, 1)
    return tuple(x[0, 0, 0].item() for x in fr.fuse(a, f, min_beams))


# ---------------------------------------------------------------- the fuse rule by hand
def test_ties_go_to_the_first_beam():
    assert _cell([3, 5, 5], [1, 1, 1], 1) == (1, 1, 5.0, 3)
    assert _cell([5, 5, 5], [0, 9, 1], 1) == (1, 1, 5.0, 2)        # the first *flagged* of the equals
    assert _cell([7, 7], [1, 1], 2) == (1, 0, 7.0, 2)


def test_min_beams_one_two_and_all():
    amps, flags = [2, 8, 3], [1, 0, 200]                            # any nonzero byte is a hit
    assert _cell(amps, flags, 1) == (1, 2, 8.0, 2)
    assert _cell(amps, flags, 2) == (1, 2, 8.0, 2)
    assert _cell(amps, flags, 3) == (0, 255, 8.0, 2)                # counted, not a hit: no peak beam
    assert _cell(amps, [1, 1, 1], 3) == (1, 1, 8.0, 3)
    assert _cell(amps, [0, 0, 0], 1) == (0, 255, 8.0, 0)


def test_a_flagged_beam_weaker_than_an_unflagged_neighbour():
    # the peak beam is the strongest flagged one; famp is the strongest of all
    assert _cell([1, 9, 4], [0, 0, 7], 1) == (1, 2, 9.0, 1)
    assert _cell([1, 9, 4], [1, 0, 1], 1) == (1, 2, 9.0, 2)


def test_famp_follows_the_stated_loop_with_negative_amplitudes():
    assert _cell([-3, -2, -5], [1, 0, 1], 1) == (1, 0, -2.0, 2)


# ---------------------------------------------------------------- the elevation rule by hand
X = [0.0, 2.0, 4.0]


def test_law_0_and_edge_beams_give_the_centre():
    for law in (0, 1, 2):
        assert fr.elev_one(law, 0, X, 0, 3, 2) == (0.0, False)
        assert fr.elev_one(law, 2, X, 2, 3, 0) == (4.0, False)
    assert fr.elev_one(0, 1, X, 1, 2, 1) == (2.0, False)


def test_law_1_by_hand_zero_and_negative_neighbours():
    assert fr.elev_one(1, 1, X, 1, 2, 1) == (2.0, True)             # (0 + 8 + 4) / 6
    assert fr.elev_one(1, 1, X, 0, 2, 2) == (3.0, True)             # (0 + 8 + 16) / 8
    assert fr.elev_one(1, 1, X, -2, 2, 0) == (1.0, True)            # squares: (0 + 8 + 0) / 8
    assert fr.elev_one(1, 1, X, 0, 0, 0) == (2.0, False)            # zero denominator
    assert fr.elev_one(1, 1, X, np.inf, 1, 1) == (2.0, False)       # infinite denominator
    assert fr.elev_one(1, 1, X, np.nan, 1, 1) == (2.0, False)


def test_law_2_by_hand():
    assert fr.elev_one(2, 1, X, 1, 2, 1) == (2.0, True)             # symmetric: the vertex is the centre
    # parabola through (0, 0), (2, ln 4), (4, ln 4): vertex half-way between the equal pair
    assert fr.elev_one(2, 1, X, 1, 4, 4) == (3.0, True)
    assert fr.elev_one(2, 1, X, 4, 4, 1) == (1.0, True)


def test_law_2_zero_negative_and_non_finite_amplitudes():
    for bad in (0.0, -1.0, np.inf, np.nan):
        for pos in range(3):
            a = [1.0, 2.0, 1.0]
            a[pos] = bad
            assert fr.elev_one(2, 1, X, *a) == (2.0, False), (bad, pos)


def test_law_2_flat_and_convex_triples():
    assert fr.elev_one(2, 1, X, 3, 3, 3) == (2.0, False)            # den = 0
    assert fr.elev_one(2, 1, X, 4, 1, 4) == (2.0, False)            # the peak beam is the weakest: convex
    assert fr.elev_one(2, 1, X, 0.25, 1, 4) == (2.0, False)        # a straight line in log: den = 0


def test_law_2_clamp():
    # ln: -4.605, 0, 1.609: vertex at 2 + 0.5 * 24.86 / 5.992 = 4.07, beyond the upper neighbour
    e, three = fr.elev_one(2, 1, X, 1e-2, 1, 5)
    assert (e, three) == (4.0, True)
    e, three = fr.elev_one(2, 1, X, 5, 1, 1e-2)
    assert (e, three) == (0.0, True)
    # inside: ln: -9.21, 0, 2.303: 2 + 0.5 * 46.05 / 13.82 = 3.67
    e, three = fr.elev_one(2, 1, X, 1e-4, 1, 10)
    assert three and e == pytest.approx(2.0 + 0.5 * (4 * math.log(10) + 4 * math.log(1e4)) / (2 * math.log(1e4) - 2 * math.log(10)), abs=1e-6)
    assert 3.6 < e < 3.7


def test_descending_centres():
    xd = [4.0, 2.0, 0.0]
    assert fr.elev_one(2, 1, xd, 1, 4, 4) == (1.0, True)            # towards beam 2, whose centre is 0
    assert fr.elev_one(1, 1, xd, 0, 2, 2) == (1.0, True)
    assert fr.elev_one(2, 1, xd, 1e-2, 1, 5) == (0.0, True)         # clamped to min(x-, x+)
    assert fr.elev_one(2, 1, xd, 4, 1, 4) == (2.0, False)


def test_elevation_walks_the_hit_list():
    amp = np.zeros((1, 3, 2, 2), np.float32)
    amp[0, :, 1, 0] = [1, 4, 4]
    flag = np.zeros((1, 3, 2, 2), np.uint8)
    flag[0, 1:, 1, 0] = 1
    fflag, fbeam, famp, fcnt = fr.fuse(amp, flag, 1)
    assert fbeam[0, 1, 0] == 1 and fflag.sum() == 1
    cells = np.array([[[1, 0], [0, 1], [5, 5], [1, 0]]], np.int32)   # a hit, a cell without one, outside, past the count
    el, hb = fr.elevation(amp, flag, fbeam, cells, np.array([[3, 0]], np.int32), X, 2)
    assert el[0, 0] == 3.0 and hb[0, 0].tolist() == [1, 2, 0, 2]
    assert np.isnan(el[0, 1]) and hb[0, 1].tolist() == [-1, 0, -1, -1]
    assert np.isnan(el[0, 2]) and hb[0, 2].tolist() == [-1, 0, -1, -1]
    assert hb[0, 3].tolist() == [-9] * 4                               # untouched


# ---------------------------------------------------------------- Gaussian beams
def test_law_2_recovers_the_elevation_of_gaussian_beams():
    """13 equal-width Gaussian beams on an uneven grid: log a is a parabola in the angle, so law 2 is exact up
    to the rounding of the float32 amplitudes and of the fp64 arithmetic.  The elevations are drawn where
    the nearest centre is an interior beam (an edge peak beam has one neighbour only and gives its centre).
    The bar 1e-5 deg is the issue's; the worst case is printed."""
    rng = np.random.default_rng(2024)
    x = np.cumsum(np.array([0.0, 2.1, 1.8, 2.3, 1.9, 2.0, 2.4, 1.7, 2.2, 1.95, 2.05, 1.85, 2.15])) - 3.0
    N = 20000
    lo, hi = 0.5 * (x[0] + x[1]) + 1e-3, 0.5 * (x[11] + x[12]) - 1e-3
    truth = rng.uniform(lo, hi, N)
    width = rng.uniform(3.0, 6.0, N)                                 # FWHM [deg], one per trial for all beams
    scale = 10.0 ** rng.uniform(-2, 4, N)
    a64 = scale[None, :] * np.exp(-4.0 * math.log(2.0) * (truth[None, :] - x[:, None]) ** 2 / width[None, :] ** 2)
    amp = a64.astype(np.float32).reshape(1, 13, 1, N)
    flag = np.ones((1, 13, 1, N), np.uint8)
    fflag, fbeam, famp, fcnt = fr.fuse(amp, flag, 13)
    assert fflag.all() and (fcnt == 13).all()
    assert (fbeam[0, 0] == np.argmin(np.abs(truth[None, :] - x[:, None]), axis=0)).all()
    cells = np.stack([np.zeros(N, np.int32), np.arange(N, dtype=np.int32)], axis=1)[None]
    el, hb = fr.elevation(amp, flag, fbeam, cells, np.array([[N, 0]], np.int32), x, 2)
    assert (hb[0, :, 2] == hb[0, :, 0] - 1).all() and (hb[0, :, 3] == hb[0, :, 0] + 1).all()
    err = np.abs(el[0] - truth)
    print("law 2 on Gaussian beams: worst |el - truth| = %.3g deg over %d trials" % (err.max(), N))
    assert err.max() < 1e-5
    # law 0 on the same hits is off by up to half a beam spacing, law 1 lies in between
    el0, _ = fr.elevation(amp, flag, fbeam, cells[:, :500], np.array([[500, 0]], np.int32), x, 0)
    el1, _ = fr.elevation(amp, flag, fbeam, cells[:, :500], np.array([[500, 0]], np.int32), x, 1)
    assert np.abs(el0[0] - truth[:500]).max() > 0.8 > 1e-5
    assert np.abs(el1[0] - truth[:500]).mean() < np.abs(el0[0] - truth[:500]).mean()


# ---------------------------------------------------------------- the C ABI's refusals
def _lib():
    from rsp import _capi as capi
    return capi, capi.load_library()


def _params(capi, beams=3, beam_el=None, **kw):
    p = capi.rsp_fuse_params()
    p.beams, p.min_beams, p.law = beams, 1, 2
    el = beam_el if beam_el is not None else [2.0 * k for k in range(beams)]
    for k, v in enumerate(el):
        p.beam_el[k] = v
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _call(lib, capi, fn="fuse", V=4, R=8, batch=2, d_amp=1 << 40, d_flag=2 << 40, params=True, d_fflag=3 << 40,
          d_fbeam=4 << 40, d_famp=5 << 40, d_fcnt=6 << 40, d_cells=7 << 40, d_count=8 << 40, max_hits=16, d_el=9 << 40,
          el_stride=3, d_hb=10 << 40, **kw):
    p = _params(capi, **kw)
    pp = C.byref(p) if params else None
    if fn == "fuse":
        rc = lib.rsp_beam_fuse_dev(None, d_amp, d_flag, V, R, batch, pp, d_fflag, d_fbeam, d_famp, d_fcnt, None)
    else:
        rc = lib.rsp_beam_elev_dev(None, d_amp, d_flag, d_fbeam, V, R, batch, pp, d_cells, d_count, max_hits, d_el,
                                   el_stride, d_hb, None)
    return rc, (lib.rsp_last_error(None) or b"").decode()


BAD = [
    ("null params", dict(params=False)),
    ("null d_amp", dict(d_amp=None)),
    ("null d_flag", dict(d_flag=None)),
    ("beams = 1", dict(beams=1)),
    ("beams = 33", dict(beams=33, beam_el=[float(k) for k in range(32)])),
    ("min_beams = 0", dict(min_beams=0)),
    ("min_beams > beams", dict(min_beams=4)),
    ("law = -1", dict(law=-1)),
    ("law = 3", dict(law=3)),
    ("reserved", dict(reserved=1)),
    ("ld < R", dict(ld=7)),
    ("V = 0", dict(V=0)),
    ("beam planes overlap", dict(beam_stride=31)),                       # a plane is 3 * 8 + 8 = 32 elements
    ("CPI planes overlap", dict(cpi_stride=95)),                         # 3 beams of 32
    ("beams inside a CPI, CPI stride short", dict(beam_stride=40, cpi_stride=111)),   # needs 2 * 40 + 32
    ("CPIs inside a beam, beam stride short", dict(beam_stride=63, cpi_stride=32)),   # needs 1 * 32 + 32
    ("interleaved", dict(beam_stride=64, cpi_stride=33)),
    ("negative beam stride", dict(beam_stride=-32)),
    ("NaN centre", dict(beam_el=[0.0, float("nan"), 4.0])),
    ("infinite centre", dict(beam_el=[0.0, 2.0, float("inf")])),
    ("equal centres", dict(beam_el=[0.0, 2.0, 2.0])),
    ("centres turn round", dict(beam_el=[0.0, 2.0, 1.0])),
    ("misaligned d_amp", dict(d_amp=(1 << 40) + 2)),
]
BAD_FUSE = [
    ("null d_fflag", dict(d_fflag=None)),
    ("null d_fbeam", dict(d_fbeam=None)),
    ("misaligned d_famp", dict(d_famp=(5 << 40) + 1)),
    ("d_fflag inside d_flag", dict(d_fflag=(2 << 40) + 5)),
    ("d_famp inside d_amp", dict(d_famp=(1 << 40) + 64)),
    ("d_fcnt is d_fbeam", dict(d_fcnt=4 << 40)),
]
BAD_ELEV = [
    ("null d_fbeam", dict(d_fbeam=None)),
    ("null d_count", dict(d_count=None)),
    ("null d_cells", dict(d_cells=None)),
    ("null d_el", dict(d_el=None)),
    ("max_hits < 0", dict(max_hits=-1)),
    ("el_stride = 0", dict(el_stride=0)),
    ("misaligned d_el", dict(d_el=(9 << 40) + 4)),
    ("misaligned d_cells", dict(d_cells=(7 << 40) + 2)),
    ("too many blocks", dict(batch=1 << 30, max_hits=1 << 20, cpi_stride=96)),
]
CASES = ([("fuse", w, k) for w, k in BAD + BAD_FUSE] + [("elev", w, k) for w, k in BAD + BAD_ELEV])


@pytest.mark.parametrize("fn,what,kw", CASES, ids=["%s-%s" % (c[0], c[1]) for c in CASES])
def test_argument_errors_before_the_context(fn, what, kw):
    capi, lib = _lib()
    rc, msg = _call(lib, capi, fn=fn, **kw)
    assert rc == capi.RSP_ERR_ARG, (what, rc, msg)
    name = "rsp_beam_fuse_dev" if fn == "fuse" else "rsp_beam_elev_dev"
    assert msg.startswith(name + ":") and "null ctx" not in msg, (what, msg)


@pytest.mark.parametrize("fn", ["fuse", "elev"])
def test_a_well_formed_call_gets_as_far_as_the_context(fn):
    capi, lib = _lib()
    ok = [dict(), dict(d_famp=None, d_fcnt=None, d_hb=None), dict(beam_el=[4.0, 2.0, 0.0]),
          dict(beam_stride=2 * 32, cpi_stride=32),                       # beam outermost: [beams][batch][V][R]
          dict(ld=10, beam_stride=50, cpi_stride=150), dict(beams=32, min_beams=32, beam_el=[-float(k) for k in range(32)]),
          dict(batch=1, beam_stride=32, cpi_stride=1),                   # one CPI: its stride is never used
          dict(law=0), dict(law=1), dict(batch=0), dict(max_hits=0, d_cells=None, d_el=None)]
    for kw in ok:
        rc, msg = _call(lib, capi, fn=fn, **kw)
        assert rc == capi.RSP_ERR_ARG and "null ctx" in msg, (kw, rc, msg)


def test_struct_layout_matches_the_header():
    capi, _ = _lib()
    P = capi.rsp_fuse_params
    assert C.sizeof(P) == 16 + 24 + 32 * 8 and capi.RSP_FUSE_MAX_BEAMS == 32
    assert [f for f, _ in P._fields_] == ["beams", "min_beams", "law", "reserved", "ld", "beam_stride", "cpi_stride", "beam_el"]
    assert (P.min_beams.offset, P.law.offset, P.reserved.offset) == (4, 8, 12)
    assert (P.ld.offset, P.beam_stride.offset, P.cpi_stride.offset, P.beam_el.offset) == (16, 24, 32, 40)
    # the header's own words
    text = open(os.path.join(ROOT, "include", "rsp.h")).read()
    body = text[text.index("#define RSP_FUSE_MAX_BEAMS 32"):text.index("} rsp_fuse_params;")]
    names = [ln.split(";")[0].split()[-1].split("[")[0] for ln in body.splitlines() if ";" in ln]
    assert names == [f for f, _ in P._fields_] and "double  beam_el[32]" in body
    assert "rsp_beam_fuse_dev" in capi.EXPORTS and "rsp_beam_elev_dev" in capi.EXPORTS


def test_the_fuser_refuses_bad_parameters_without_a_gpu():
    from rsp import _capi as capi
    from rsp.fuse import BeamFuser
    with pytest.raises(capi.RspError, match="min_beams"):
        BeamFuser([0.0, 2.0, 4.0], min_beams=4)
    with pytest.raises(capi.RspError, match="monotonic"):
        BeamFuser([0.0, 2.0, 2.0])
    with pytest.raises(ValueError, match="law"):
        BeamFuser([0.0, 2.0, 4.0], law="spline")
    with pytest.raises(ValueError, match="beam centres"):
        BeamFuser([0.0])


# ---------------------------------------------------------------- the kernel's arithmetic header on the host
@pytest.fixture(scope="module")
def math_check(tmp_path_factory):
    """tests/native/fuse_math_check.cpp through its makefile (tests/native/fuse_math_check.mk): the header
    elev_kernel compiles, as a host program (contraction off), plain and with -fsanitize=address,undefined."""
    out = str(tmp_path_factory.mktemp("fm"))
    exes = [os.path.join(out, n) for n in ("fuse_math_check", "fuse_math_check_san")]
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "native"), "-f", "fuse_math_check.mk", "OUT=" + out] + exes,
                   check=True, capture_output=True, text=True, timeout=300)
    return exes


def _records():
    rng = np.random.default_rng(99)
    xs = {3: X, -3: [4.0, 2.0, 0.0],
          13: list(np.cumsum([0.0, 2.1, 1.8, 2.3, 1.9, 2.0, 2.4, 1.7, 2.2, 1.95, 2.05, 1.85, 2.15]) - 3.0),
          32: [-1.5 * k for k in range(32)]}
    designed = [(1, 2, 1), (1, 4, 4), (4, 4, 1), (3, 3, 3), (4, 1, 4), (1e-3, 1, 1e3), (1e-2, 1, 5), (5, 1, 1e-2), (1e-4, 1, 10),
                (0, 2, 2), (-2, 2, 0), (0, 0, 0), (np.inf, 1, 1), (1, np.inf, 1), (np.nan, 1, 1), (1, 1, np.nan), (1, 0, 1),
                (1, -1, 1), (1e-38, 1e-30, 1e-38), (3e38, 3e38, 1e38), (1e-45, 1e-44, 1e-45), (2, 2, 1), (1, 2, 2)]
    recs = []
    for law in (0, 1, 2):
        for key, x in xs.items():
            n = len(x)
            for k in sorted({0, 1, n // 2, n - 2, n - 1}):
                for a in designed:
                    recs.append((law, k, x, a))
            for _ in range(60):
                k = int(rng.integers(0, n))
                a = tuple(np.abs(rng.standard_normal(3)).astype(np.float32) * 10.0 ** rng.integers(-3, 4))
                recs.append((law, k, x, a))
    return recs


def test_header_arithmetic_gives_the_restatements_bits(math_check, tmp_path):
    recs = _records()
    payload = b"".join(struct.pack("<4i32d4f", law, k, len(x), 0, *(list(x) + [0.0] * (32 - len(x))),
                                   *[float(np.float32(v)) for v in a], 0.0) for law, k, x, a in recs)
    want = [fr.elev_one(law, k, x, *a) for law, k, x, a in recs]
    assert sum(t for _, t in want) > len(recs) // 4 and sum(not t for _, t in want) > len(recs) // 4
    src = str(tmp_path / "in.bin")
    with open(src, "wb") as f:
        f.write(payload)
    for exe in math_check:
        dst = str(tmp_path / (os.path.basename(exe) + ".out"))
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (exe, r.returncode, r.stderr[-2000:])
        got = np.fromfile(dst, dtype=np.dtype([("bits", "<u8"), ("three", "<i4"), ("pad", "<i4")]))
        assert len(got) == len(recs)
        for (law, k, x, a), (e, three), g in zip(recs, want, got):
            assert int(g["three"]) == int(three), (exe, law, k, a)
            assert int(g["bits"]) == struct.unpack("<Q", struct.pack("<d", e))[0], (exe, law, k, x, a, e)
