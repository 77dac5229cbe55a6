"""rsp_condense_dev on the GPU against the restatement tests/condense_ref.py, on designed scenes.
Every comparison is exact integer equality: the tie rule makes every output unique.

Each scene is a batch of CPIs in one of four layouts:
  A  33 x 17, ld = R (odd sizes, the byte path of the dense pass)
  B  96 x 130 as a window at column 7 of ld = 160 planes, the CPI stride padded by 48
  C  192 x 96, ld = R (16-byte path; several tiles of rows)
  D  one 2048 x 574 CPI condensed as the two DMX windows (0, 62) and (62, 574)
The references are computed once per scene and shared (module cache).
"""
import ctypes as C

import numpy as np
import pytest

import condense_ref

pytestmark = pytest.mark.gpu

SENT_U8, SENT_I32 = 0xAB, -7777
LAYOUTS = {"A": (33, 17, 17, 0, 0), "B": (96, 130, 160, 7, 48), "C": (192, 96, 96, 0, 0)}   # V, R, ld, col0, pad


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from rsp.condense import Condense
    from rsp.measure import Measure
    c, m = Condense(0), Measure(0)
    yield c, m
    c.close()
    m.close()


def _run(gpu, amp, flag, V, R, ld, col0, pad, gap, wrap_v, max_plots, with_plots=True, measure=True, peak_shift=0):
    """amp / flag: [B][V][R] windows.  Places them in [B] planes of pitch ld (+ pad elements
    between CPIs) at column col0, everything else sentinel, and returns the whole peak buffer,
    the plots buffer, the counts and the measurement's cells of the peak plane."""
    import torch
    from rsp import _capi as capi
    cond, meas = gpu
    B = amp.shape[0]
    cs = V * ld + pad
    a_full = np.full((B, cs), 3.5, np.float32)
    f_full = np.ones((B, cs), np.uint8)            # hits all around the window: they must not join in
    for b in range(B):
        av = a_full[b, :V * ld].reshape(V, ld)
        fv = f_full[b, :V * ld].reshape(V, ld)
        av[:, col0:col0 + R] = amp[b]
        fv[:, col0:col0 + R] = flag[b]
    d_a = torch.from_numpy(a_full).cuda()
    d_f = torch.from_numpy(f_full).cuda()
    # peak_shift: the peak planes start that many bytes off the flag planes' 16-byte alignment
    d_peak_buf = torch.full((B * cs + 16,), SENT_U8, dtype=torch.uint8, device="cuda")
    d_peak = d_peak_buf[peak_shift:peak_shift + B * cs].view(B, cs)
    d_plots = torch.full((B, max(max_plots, 1), 8), SENT_I32, dtype=torch.int32, device="cuda")
    d_count = torch.full((B, 2), SENT_I32, dtype=torch.int32, device="cuda")
    p = capi.rsp_condense_params()
    p.gap_v, p.gap_r, p.wrap_v, p.ld, p.cpi_stride = gap[0], gap[1], int(wrap_v), ld, cs
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi.check(cond.lib.rsp_condense_dev(cond.ctx, d_a.data_ptr() + 4 * col0, d_f.data_ptr() + col0, V, R, B, C.byref(p),
                                         d_peak.data_ptr() + col0, max_plots,
                                         d_plots.data_ptr() if with_plots else None, d_count.data_ptr(), st), cond.ctx)
    cells = None
    if measure:
        mp = meas.params(1, 1.0, 2, 1.0, 2, 1.0, 0, 5.0, 0.0, 0.0, 0)
        mp.ld, mp.cpi_stride = ld, cs
        rs = torch.arange(R, dtype=torch.float64, device="cuda")
        vs = torch.arange(V, dtype=torch.float64, device="cuda")
        mh = max(max_plots, 1)
        d_est = torch.empty((B, mh, 3), dtype=torch.float64, device="cuda")
        d_cells = torch.full((B, mh, 2), SENT_I32, dtype=torch.int32, device="cuda")
        d_mc = torch.empty((B, 2), dtype=torch.int32, device="cuda")
        capi.check(meas.lib.rsp_motion_measure_dev(meas.ctx, d_a.data_ptr() + 4 * col0, d_a.data_ptr() + 4 * col0,
                                                   d_peak.data_ptr() + col0, V, R, B, C.byref(mp), rs.data_ptr(),
                                                   vs.data_ptr(), mh, d_est.data_ptr(), d_cells.data_ptr(),
                                                   d_mc.data_ptr(), st), meas.ctx)
        cells = (d_cells, d_mc)
    torch.cuda.synchronize()
    if measure:
        cells = (cells[0].cpu().numpy(), cells[1].cpu().numpy())
    slack = d_peak_buf.cpu().numpy()
    assert (slack[:peak_shift] == SENT_U8).all() and (slack[peak_shift + B * cs:] == SENT_U8).all()
    return d_peak.cpu().numpy(), d_plots.cpu().numpy(), d_count.cpu().numpy(), cells


_REFS = {}


def _ref(key, amp, flag, gap, wrap_v):
    if key not in _REFS:
        _REFS[key] = [condense_ref.condense(amp[b], flag[b], gap=gap, wrap_v=wrap_v) for b in range(amp.shape[0])]
    return _REFS[key]


def _check(gpu, key, layout, amp, flag, gap, wrap_v, max_plots=None, with_plots=True, peak_shift=0):
    V, R, ld, col0, pad = LAYOUTS[layout] if isinstance(layout, str) else layout
    B = amp.shape[0]
    refs = _ref(key, amp, flag, gap, wrap_v)
    if max_plots is None:
        max_plots = max(r[2][0] for r in refs) + 3
    peak, plots, count, cells = _run(gpu, amp, flag, V, R, ld, col0, pad, gap, wrap_v, max_plots, with_plots,
                                     peak_shift=peak_shift)
    cs = V * ld + pad
    want_peak = np.full((B, cs), SENT_U8, np.uint8)
    want_plots = np.full((B, max(max_plots, 1), 8), SENT_I32, np.int32)
    for b, (rp, rpl, (n_plots, n_hits)) in enumerate(refs):
        want_peak[b, :V * ld].reshape(V, ld)[:, col0:col0 + R] = rp
        w = min(n_plots, max_plots) if with_plots else 0
        want_plots[b, :w] = rpl[:w]
        assert tuple(count[b]) == (n_plots, n_hits), (key, b)
        # the measurement lists the peak plane's hits in the order of the plots
        assert cells[1][b, 0] == n_plots
        wm = min(n_plots, max(max_plots, 1))
        np.testing.assert_array_equal(cells[0][b, :wm], rpl[:wm, :2], err_msg="%s cpi %d" % (key, b))
    # the window matches and nothing outside it (other columns, row padding, CPI padding) is touched
    np.testing.assert_array_equal(peak, want_peak, err_msg=key)
    # the first min(n, max_plots) records match and the sentinel fill behind them is intact
    np.testing.assert_array_equal(plots, want_plots, err_msg=key)
    return peak, plots, count


def _amps(rng, shape, levels=None):
    a = rng.random(shape).astype(np.float32) + 0.25
    if levels:
        a = (np.floor(a * levels) / levels + 0.5).astype(np.float32)
    return a


def _random(seed, layout, density, levels=(None, 4, None)):
    V, R = LAYOUTS[layout][:2]
    rng = np.random.default_rng(seed)
    flag = (rng.random((3, V, R)) < density).astype(np.uint8)
    amp = np.stack([_amps(rng, (V, R), lv) for lv in levels])
    return amp, flag


def test_isolated_block_serpentine(gpu):
    """192 x 96, gap (1, 1): isolated hits on a 3-cell grid; a solid block; a one-cell-wide
    serpentine of vertical arms in the even columns, joined alternately at the bottom and the top
    row, that visits every row: one plot with long union chains."""
    V, R = LAYOUTS["C"][:2]
    rng = np.random.default_rng(1)
    flag = np.zeros((3, V, R), np.uint8)
    flag[0, ::3, ::3] = 1
    flag[1, 40:101, 10:71] = 1
    flag[2, :, 0::2] = 1
    for c in range(1, R - 1, 2):
        flag[2, V - 1 if c % 4 == 1 else 0, c] = 1
    amp = _amps(rng, (3, V, R))
    peak, plots, count = _check(gpu, "iso-block-serp", "C", amp, flag, (1, 1), False)
    assert count[0, 0] == count[0, 1] == 64 * 32
    assert tuple(count[1]) == (1, 61 * 61) and plots[1, 0, 2] == 61 * 61
    assert tuple(count[2]) == (1, V * (R // 2) + R // 2 - 1) and tuple(plots[2, 0, 3:7]) == (0, V - 1, 0, R - 2)


def test_late_u_empty_full(gpu):
    """33 x 17: a U whose arms meet only in the last row (the equivalence is resolved late), the
    empty plane (count 0, an all-zero peak plane) and the full plane (one plot of V*R cells)."""
    V, R = LAYOUTS["A"][:2]
    rng = np.random.default_rng(2)
    flag = np.zeros((3, V, R), np.uint8)
    flag[0, :, 2] = flag[0, :, 14] = 1
    flag[0, V - 1, 2:15] = 1
    flag[2] = 1
    amp = _amps(rng, (3, V, R))
    peak, plots, count = _check(gpu, "u-empty-full", "A", amp, flag, (1, 1), False)
    assert tuple(count[0]) == (1, 2 * V + 11)
    assert tuple(count[1]) == (0, 0) and peak[1].sum() == 0
    assert tuple(count[2]) == (1, V * R) and tuple(plots[2, 0, 2:]) == (V * R, 0, V - 1, 0, R - 1, 0)


def test_full_plane_many_tiles(gpu):
    """192 x 96 fully flagged, all amplitudes equal but one plateau of three: one plot of V*R
    cells whose peak is the plateau's first cell in find() order (expected values written out,
    no search)."""
    V, R = LAYOUTS["C"][:2]
    amp = np.ones((3, V, R), np.float32)
    flag = np.ones((3, V, R), np.uint8)
    amp[1, 100, 50] = amp[1, 99, 51] = amp[1, 7, 52] = 2.0
    amp[2, V - 1, R - 1] = 4.0
    peak, plots, count, cells = _run(gpu, amp, flag, V, R, R, 0, 0, (1, 1), False, 4)
    for b, (pv, pr) in enumerate(((0, 0), (100, 50), (V - 1, R - 1))):
        assert tuple(count[b]) == (1, V * R)
        assert plots[b, 0].tolist() == [pv, pr, V * R, 0, V - 1, 0, R - 1, 0]
        assert (plots[b, 1:] == SENT_I32).all()
        want = np.zeros((V, R), np.uint8)
        want[pv, pr] = 1
        np.testing.assert_array_equal(peak[b].reshape(V, R), want)
        assert cells[0][b, 0].tolist() == [pv, pr]


@pytest.mark.parametrize("gap", [(1, 1), (2, 1), (0, 3), (4, 4)])
def test_pairs_at_gap_and_gap_plus_one(gpu, gap):
    """33 x 17: CPI 0 holds a pair exactly `gap` apart in each axis (each one plot, where the gap
    is not 0), CPI 1 the same pairs gap+1 apart (two plots each), CPI 2 a random plane."""
    V, R = LAYOUTS["A"][:2]
    rng = np.random.default_rng(10 + gap[0] * 5 + gap[1])
    flag = np.zeros((3, V, R), np.uint8)
    for b, extra in ((0, 0), (1, 1)):
        flag[b, 2, 2] = flag[b, 2 + gap[0] + extra, 2] = 1
        flag[b, 22, 3] = flag[b, 22, 3 + gap[1] + extra] = 1
    flag[2] = rng.random((V, R)) < 0.3
    amp = _amps(rng, (3, V, R))
    peak, plots, count = _check(gpu, "pairs-%d-%d" % gap, "A", amp, flag, gap, False)
    assert count[0, 0] == 2 and count[1, 0] == 4


@pytest.mark.parametrize("wrap_v", [0, 1])
@pytest.mark.parametrize("gap", [(1, 1), (2, 1)])
def test_seam(gpu, gap, wrap_v):
    """33 x 17: a pair on rows 0 and V-1, a diagonal across the seam, and a random plane."""
    V, R = LAYOUTS["A"][:2]
    rng = np.random.default_rng(30)
    flag = np.zeros((3, V, R), np.uint8)
    flag[0, 0, 4] = flag[0, V - 1, 4] = 1
    flag[0, V - gap[0], 9] = flag[0, 0, 10] = 1
    flag[1, V - 2, 2] = flag[1, V - 1, 3] = flag[1, 0, 4] = flag[1, 1, 5] = 1
    flag[2] = rng.random((V, R)) < 0.25
    amp = _amps(rng, (3, V, R))
    peak, plots, count = _check(gpu, "seam-%d-%d-%d" % (gap + (wrap_v,)), "A", amp, flag, gap, bool(wrap_v))
    assert count[0, 0] == (2 if wrap_v else 4) and count[1, 0] == (1 if wrap_v else 2)
    if wrap_v:
        assert tuple(plots[1, 0, 3:5]) == (0, V - 1)       # plain minima and maxima across the seam


@pytest.mark.parametrize("density", [0.01, 0.06, 0.30, 0.45, 0.60])
def test_random_window(gpu, density):
    """96 x 130 at column 7 of ld = 160 planes with a padded CPI stride: float32 random amplitudes
    (CPIs 0, 2) and amplitudes quantised to 4 levels, so many ties (CPI 1)."""
    amp, flag = _random(round(density * 100), "B", density)
    _check(gpu, "random-B-%g" % density, "B", amp, flag, (1, 1), False)


@pytest.mark.parametrize("layout,gap,wrap_v,density", [("C", (1, 1), True, 0.06), ("C", (2, 1), False, 0.06),
                                                       ("B", (0, 3), True, 0.30), ("A", (4, 4), True, 0.06),
                                                       ("C", (0, 0), False, 0.30)])
def test_random_other_gaps(gpu, layout, gap, wrap_v, density):
    amp, flag = _random(77, layout, density, levels=(None, 4, 4))
    _check(gpu, "random-%s-%d-%d-%d-%g" % ((layout,) + gap + (wrap_v, density)), layout, amp, flag, gap, wrap_v)


@pytest.mark.parametrize("layout,density", [("A", 0.30), ("B", 0.06), ("C", 0.06)])
def test_peak_plane_off_the_flags_alignment(gpu, layout, density):
    """The peak planes 3 bytes off the flag planes' 16-byte alignment: the dense pass's byte path
    (the other tests run its aligned-granule path, also at odd pitches and window columns)."""
    amp, flag = _random(91, layout, density)
    _check(gpu, "shift-%s" % layout, layout, amp, flag, (1, 1), layout == "C", peak_shift=3)


def test_overflow_and_null_plots(gpu):
    """max_plots below the plot count: the counts are total, the first max_plots records right,
    the sentinel behind them untouched and the peak plane complete; d_plots == NULL likewise."""
    amp, flag = _random(6, "B", 0.06)
    key = "random-B-0.06"
    refs = _ref(key, amp, flag, (1, 1), False)
    assert min(r[2][0] for r in refs) > 5
    _check(gpu, key, "B", amp, flag, (1, 1), False, max_plots=5)
    _check(gpu, key, "B", amp, flag, (1, 1), False, max_plots=0)
    V, R, ld, col0, pad = LAYOUTS["B"]
    peak, plots, count, _ = _run(gpu, amp, flag, V, R, ld, col0, pad, (1, 1), False, 5, with_plots=False, measure=False)
    full = _run(gpu, amp, flag, V, R, ld, col0, pad, (1, 1), False, 4096, measure=False)
    np.testing.assert_array_equal(peak, full[0])
    np.testing.assert_array_equal(count, full[2])
    assert (plots == SENT_I32).all()


def test_runs_identical_and_batch_independent(gpu):
    """Two runs give the same bytes, and each CPI alone gives its slice of the batch."""
    amp, flag = _random(45, "B", 0.45, levels=(4, 4, None))
    V, R, ld, col0, pad = LAYOUTS["B"]
    r1 = _run(gpu, amp, flag, V, R, ld, col0, pad, (1, 1), True, 1500, measure=False)
    r2 = _run(gpu, amp, flag, V, R, ld, col0, pad, (1, 1), True, 1500, measure=False)
    for x, y in zip(r1[:3], r2[:3]):
        assert x.tobytes() == y.tobytes()
    for b in range(3):
        one = _run(gpu, amp[b:b + 1], flag[b:b + 1], V, R, ld, col0, pad, (1, 1), True, 1500, measure=False)
        for x, y in zip(r1[:3], one[:3]):
            assert x[b].tobytes() == y[0].tobytes()


def test_dmx_windows_exceed_one_tile(gpu):
    """One 2048 x 574 CPI condensed as the DMX windows (0, 62) and (62, 574) of the same planes.
    THE case that exceeds one workgroup's dense tile in both axes: a tile is 64 rows x 16
    memory-aligned 16-byte granules, the long window spans 33 granules (3 tiles) by 2048 rows (32
    tiles).  Clusters straddle the tile borders (rows 63|64; the 256-byte border, which lies at
    window column 241..256 depending on the row's address) and their corner, and hits on both
    sides of column 61|62 must not join across the windows."""
    V, Rp = 2048, 574
    rng = np.random.default_rng(5)
    flag = (rng.random((1, V, Rp)) < 0.004).astype(np.uint8)
    flag[0, 58:70, 62 + 236:62 + 262] = 1              # across the corner of four tiles
    flag[0, 63:65, 62 + 100] = 1                       # across a row border
    flag[0, 700, 62 + 238:62 + 259] = 1                # across a column border
    flag[0, 1000:1003, 60:64] = 1                      # across the short | long edge
    flag[0, 0, 300] = flag[0, V - 1, 300] = 1          # the seam (no wrap here)
    amp = _amps(rng, (1, V, Rp), 8)
    import torch
    cond, _ = gpu
    d_a, d_f = torch.from_numpy(amp).cuda(), torch.from_numpy(flag).cuda()
    d_peak = torch.full((1, V, Rp), SENT_U8, dtype=torch.uint8, device="cuda")
    outs = {}
    for cols in ((0, 62), (62, 574)):
        _, plots, count = cond.condense_dev(d_a, d_f, gap=(1, 1), wrap_v=False, max_plots=8192, cols=cols, peak=d_peak)
        outs[cols] = (plots, count)
    torch.cuda.synchronize()
    peak = d_peak.cpu().numpy()
    for (lo, hi), (plots, count) in outs.items():
        rp, rpl, (n_plots, n_hits) = condense_ref.condense(amp[0, :, lo:hi], flag[0, :, lo:hi], gap=(1, 1))
        assert tuple(count.cpu().numpy()[0]) == (n_plots, n_hits)
        np.testing.assert_array_equal(peak[0, :, lo:hi], rp)
        np.testing.assert_array_equal(plots.cpu().numpy()[0, :n_plots], rpl)
    # the block across the windows' edge is one plot on each side
    assert peak[0, 1000:1003, 60:62].sum() == 1 and peak[0, 1000:1003, 62:64].sum() == 1


@pytest.fixture(scope="module")
def dmx():
    import torch
    from rsp.dmx import DmxFrameProcessor
    proc = DmxFrameProcessor(freInd=2)
    from rsp import presets
    spec = proc.spec
    rng = np.random.default_rng(77)
    e = (rng.standard_normal((2, 2, spec.P, spec.R)) + 1j * rng.standard_normal((2, 2, spec.P, spec.R))) * np.sqrt(0.5)
    rep = presets.load_data("refDDCDataMF1").astype(np.complex128).ravel()
    sig = 0.5 * np.exp(2j * np.pi * 0.13 * np.arange(spec.P)[:, None]) * rep[None, :] / np.abs(rep).max()
    e[:, 0, :, 62 + 200:62 + 200 + rep.size] += sig
    e[:, 1, :, 62 + 200:62 + 200 + rep.size] += 0.7 * sig
    echo = torch.from_numpy(e.astype(np.complex64)).cuda()
    yield proc, echo
    proc.close()


def test_process_dev_condensed(gpu, dmx):
    """process_dev(condense=...) on the two-beam DMX engine, two frames of noise and one target (the
    scene of test_gpu_measure.py's test_dmx_frame_processor): per part and flag kind,
    the peak planes and plots are the restatement's on the chain's own flags, and the estimates
    are what measure_dev gives on the restatement's peak plane."""
    import torch
    proc, echo = dmx
    out = proc.process_dev(echo, beamPosNum=4, max_hits=4096, condense=dict(gap=(1, 1)))
    torch.cuda.synchronize()
    s = out["sum"].cpu().numpy()
    rS, rL, vS = proc.scales[:3]
    o = proc.o
    p = proc.meas.params(o["extraDots"], proc.scales[3], o["rInterpTimes"], proc.scales[4], o["vInterpTimes"],
                         float(proc.kValues[2, 4]), 4, o["beamAngleStep"], o["eleAngleComp"], o["eleAngleSysErr"],
                         proc.spec.radar["M0"])
    for fk, pk in (("flag", "peak"), ("flagV", "peakV")):
        f = out[fk].cpu().numpy()
        want_peak = np.zeros_like(f)
        for part, (lo, hi), rsc in (("short", (0, 62), rS), ("long", (62, 574), rL)):
            plots, count = (t.cpu().numpy() for t in out[(part, fk, "plots")])
            for b in range(f.shape[0]):
                rp, rpl, n = condense_ref.condense(s[b, :, lo:hi], f[b, :, lo:hi], gap=(1, 1))
                assert n[0] <= 4096
                if (part, fk) == ("long", "flag"):
                    assert 0 < n[0] < n[1]                           # the target: clusters, not single cells
                want_peak[b, :, lo:hi] = rp
                assert tuple(count[b]) == n
                np.testing.assert_array_equal(plots[b, :n[0]], rpl)
            est, cells, mcount = proc.meas.measure_dev(out["sum"], out["diff"], torch.from_numpy(want_peak).cuda(), p,
                                                       rsc, vS, max_hits=4096, cols=(lo, hi))
            got = out[(part, fk)]
            torch.cuda.synchronize()
            assert torch.equal(mcount, got[2])
            for b in range(f.shape[0]):
                k = int(mcount[b, 0])
                assert got[0][b, :k].cpu().numpy().tobytes() == est[b, :k].cpu().numpy().tobytes()
                assert torch.equal(got[1][b, :k], cells[b, :k])
        np.testing.assert_array_equal(out[pk].cpu().numpy(), want_peak)


def test_process_dev_default_unchanged(gpu, dmx):
    """Without the argument (and with condense=None): the keys of before, no peak planes, and per
    part and kind the bytes measure_dev gives on the chain's own flags, every hit measured."""
    import torch
    proc, echo = dmx
    parts = [(a, b) for a in ("short", "long") for b in ("flag", "flagV")]
    rS, rL, vS = proc.scales[:3]
    o = proc.o
    p = proc.meas.params(o["extraDots"], proc.scales[3], o["rInterpTimes"], proc.scales[4], o["vInterpTimes"],
                         float(proc.kValues[2, 4]), 4, o["beamAngleStep"], o["eleAngleComp"], o["eleAngleSysErr"],
                         proc.spec.radar["M0"])
    for kw in ({}, dict(condense=None)):
        out = proc.process_dev(echo, beamPosNum=4, **kw)
        torch.cuda.synchronize()
        assert set(out) == {"sum", "diff", "flag", "flagV"} | set(parts)
        for part, fk in parts:
            cols, rsc = ((0, 62), rS) if part == "short" else ((62, 574), rL)
            est, cells, count = proc.meas.measure_dev(out["sum"], out["diff"], out[fk], p, rsc, vS, max_hits=4096,
                                                      cols=cols)
            torch.cuda.synchronize()
            got = out[(part, fk)]
            assert got[0].shape == est.shape and torch.equal(got[2], count)
            assert (part, fk) != ("long", "flag") or int(count[:, 0].min()) > 0
            for b in range(count.shape[0]):
                w = min(int(count[b, 0]), est.shape[1])
                assert got[0][b, :w].cpu().numpy().tobytes() == est[b, :w].cpu().numpy().tobytes()
                assert torch.equal(got[1][b, :w], cells[b, :w])
