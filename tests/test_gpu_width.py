"""Doppler line width on the GPU (rsp_spec_width_dev, csrc/rsp_width.hip) against the fp64
restatement tests/width_ref.py.  Spans are compared as exact integers on every computed column
that is not a tie column (margin <= 1e-9 of M1; tests/test_width_cpu.py asserts that these scenes
have none); uncomputed columns must read {-1, -1} and the count must be exact.  A test fails if
it leaves out more than 1 % of its computed columns.
"""
import ctypes as C
import os

import numpy as np
import pytest

import width_ref as wr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def wd():
    from rsp.width import Width
    w = Width(0)
    yield w
    w.close()


def _check(tested, ties):
    assert tested > 0
    assert ties <= wr.TIE_CAP * tested, "%d of %d computed columns are ties" % (ties, tested)


def _column_flags(V, R):
    """One hit in every column but each third (c % 3 == 2), in a row that moves with the column."""
    f = np.zeros((V, R), np.uint8)
    for c in range(R):
        if c % 3 != 2:
            f[(5 * c + 1) % V, c] = 1
    return f


@pytest.mark.parametrize("V,R", wr.SHAPES, ids=["%dx%d" % s for s in wr.SHAPES])
def test_shapes_interp_levels_shift(wd, V, R):
    """Every V (4 and 5: the smallest general spline and the odd rotation; 332: no power of two;
    2048: the longest) at every interp, level and shift, ld = R, hits in two columns of three."""
    import torch
    amp = wr.scene(V, R, seed=V)
    flag = _column_flags(V, R)
    need = flag.any(axis=0)
    d_amp, d_flag = torch.from_numpy(amp).cuda(), torch.from_numpy(flag).cuda()
    tested = ties = 0
    for interp in wr.interps_for(V):
        for shift in (0, 1):
            x, s = wr.samples(amp[:, need], interp, True, bool(shift))
            for lv in wr.LEVELS:
                span, count = wd.width_dev(d_amp, d_flag, lv, interp, shift)
                span, count = span.cpu().numpy()[0], int(count.cpu()[0])
                assert count == int(need.sum())
                assert (span[~need] == -1).all()
                first, last, _, margin = wr.select(x, s, lv, interp)
                ok = margin > wr.TIE
                got = span[need]
                bad = ok & ((got[:, 0] != first) | (got[:, 1] != last))
                assert not bad.any(), (interp, shift, lv, got[bad][:4].tolist(), first[bad][:4].tolist(),
                                       last[bad][:4].tolist(), margin[bad][:4].tolist())
                tested += int(ok.size)
                ties += int((~ok).sum())
    _check(tested, ties)


def _window_buffers(flag_planes):
    """The 96 x 130 window at column 7 of ld = 160 planes with a padded CPI stride: amplitudes
    outside the window are huge and flags outside it are set, so neither may be looked at."""
    import torch
    w = wr.WIN
    V, R, c0, ld, cs, B = w["V"], w["R"], w["col0"], w["ld"], w["cs"], w["batch"]
    amp = np.full(B * cs + 64, 3.0e30, np.float32)
    flag = np.full(B * cs + 64, 1, np.uint8)
    scenes = []
    for b in range(B):
        a = wr.scene(V, R, seed=70 + b)
        scenes.append(a)
        rows = b * cs + np.arange(V)[:, None] * ld + c0 + np.arange(R)[None, :]
        amp[rows] = a
        flag[rows] = flag_planes[b] if flag_planes is not None else 1
    return scenes, amp, flag, torch.from_numpy(amp).cuda(), torch.from_numpy(flag).cuda()


def _raw(wd, d_amp, d_flag, B, lv, interp, shift, first_cpi=0):
    """rsp_spec_width_dev on the window buffers, the outputs inside guarded arrays."""
    import torch
    from rsp import _capi as capi
    w = wr.WIN
    V, R, c0, ld, cs = w["V"], w["R"], w["col0"], w["ld"], w["cs"]
    G = 16
    span = torch.full((G + B * R * 2 + G,), -77, dtype=torch.int32, device="cuda")
    count = torch.full((G + B + G,), -77, dtype=torch.int32, device="cuda")
    p = capi.rsp_width_params()
    p.amp_constr, p.interp, p.shift, p.ld, p.cpi_stride = lv, interp, shift, ld, cs
    off = first_cpi * cs + c0
    st = torch.cuda.current_stream().cuda_stream
    capi.check(wd.lib.rsp_spec_width_dev(
        wd.ctx, d_amp.data_ptr() + 4 * off, None if d_flag is None else d_flag.data_ptr() + off, V, R, B, C.byref(p),
        span.data_ptr() + 4 * G, count.data_ptr() + 4 * G, C.c_void_p(st)), wd.ctx)
    torch.cuda.synchronize()
    span, count = span.cpu().numpy(), count.cpu().numpy()
    assert (span[:G] == -77).all() and (span[-G:] == -77).all(), "written outside d_span"
    assert (count[:G] == -77).all() and (count[-G:] == -77).all(), "written outside d_count"
    return span[G:-G].reshape(B, R, 2), count[G:-G]


@pytest.mark.parametrize("mode", ["none", "edges", "random", "null"])
def test_window_with_padded_stride(wd, mode):
    """Batch 3 over the window case: no hit at all, hits in single columns at both window edges
    and either side of the column-group boundaries, random hits, and d_flag = NULL.  Nothing but
    d_span and d_count is written, CPI 1 alone gives its bytes in the batch, two runs agree."""
    w = wr.WIN
    V, R, B = w["V"], w["R"], w["batch"]
    if mode == "none":
        planes = [np.zeros((V, R), np.uint8)] * B
    elif mode == "edges":
        f, cols = wr.edge_flags(V, R)
        assert {0, 15, 16, 63, 64, R - 1} <= set(cols)
        planes = [f, f[::-1].copy(), np.roll(f, 1, axis=1)]
    elif mode == "random":
        planes = [wr.sparse_flags(V, R, 40, seed=5 + b) for b in range(B)]
    else:
        planes = None
    scenes, amp, flag, d_amp, d_flag = _window_buffers(planes)
    tested = ties = 0
    for interp, shift in ((4, 1), (3, 0)):
        for lv in wr.LEVELS if mode in ("null", "random") else (-6.0,):
            span, count = _raw(wd, d_amp, None if planes is None else d_flag, B, lv, interp, shift)
            for b in range(B):
                need = np.ones(R, bool) if planes is None else planes[b].any(axis=0)
                t, k = wr.compare(span[b], count[b], scenes[b], need, lv, interp, bool(shift))
                tested, ties = tested + t, ties + k
            again, count2 = _raw(wd, d_amp, None if planes is None else d_flag, B, lv, interp, shift)
            assert again.tobytes() == span.tobytes() and count2.tobytes() == count.tobytes()
            one, count1 = _raw(wd, d_amp, None if planes is None else d_flag, 1, lv, interp, shift, first_cpi=1)
            assert one[0].tobytes() == span[1].tobytes() and count1[0] == count[1]
    np.testing.assert_array_equal(d_amp.cpu().numpy(), amp)
    np.testing.assert_array_equal(d_flag.cpu().numpy(), flag)
    if mode == "none":
        assert tested == 0 and (span == -1).all() and (count == 0).all()
    else:
        _check(tested, ties)


def test_all_zero_and_constant_columns(wd):
    """A computed column whose maximum is not positive reads {-1, -1} and still counts; a
    constant column spans everything."""
    import torch
    V, R = 33, 5
    amp = wr.scene(V, R, seed=3)
    amp[:, 1] = 0.0
    amp[:, 3] = 2.5
    span, count = wd.width_dev(torch.from_numpy(amp).cuda(), None, -6.0, 4, 1)
    span = span.cpu().numpy()[0]
    assert int(count.cpu()[0]) == R
    assert span[1].tolist() == [-1, -1] and span[3].tolist() == [0, (V - 1) * 4]
    wr.compare(span, R, amp, np.ones(R, bool), -6.0, 4, True)


def test_dmx_windows(wd):
    """One 2048 x 574 CPI as the DMX short (0, 62) and long (62, 574) windows of the same planes,
    about 1044 hits, interp 4 and 8 at -6 dB with the fftshift these planes lack."""
    import torch
    d = wr.DMX
    V, Rp = d["V"], d["Rp"]
    amp = wr.scene(V, Rp, seed=2048574)
    flag = wr.sparse_flags(V, Rp, d["hits"], seed=11)
    d_amp, d_flag = torch.from_numpy(amp).cuda(), torch.from_numpy(flag).cuda()
    tested = ties = 0
    for interp in (4, 8):
        for lo, hi in d["windows"]:
            span, count = wd.width_dev(d_amp, d_flag, -6.0, interp, 1, cols=(lo, hi))
            t, k = wr.compare(span.cpu().numpy()[0], int(count.cpu()[0]), amp[:, lo:hi], flag[:, lo:hi].any(axis=0),
                              -6.0, interp, True)
            tested, ties = tested + t, ties + k
    _check(tested, ties)
    assert tested > 800


def test_ampConstrWidthEst(wd):  # noqa: N802 (reference name)
    """The reference-named entry against the restatement: complex and real, 1-D and 2-D, with and
    without interpFlag."""
    import rsp
    rng = np.random.default_rng(8)
    a = wr.scene(128, 6, seed=21).astype(np.float64)
    spec = a * np.exp(2j * np.pi * rng.uniform(size=a.shape))
    mag = np.abs(spec).astype(np.float32)                  # what the host hands to the kernel
    for lv, flag, interp in ((-6.0, 1, 8), (-3.0, 0, 8), (-20.0, 1, 1), (-40.0, 1, 3)):
        _, _, want, margin = wr.width(mag, lv, flag, interp)
        assert (margin > wr.TIE).all()
        got = wd.ampConstrWidthEst(spec, lv, flag, interp)
        assert got.dtype == np.float64 and got.shape == (6,)
        np.testing.assert_array_equal(got, want)
        one = wd.ampConstrWidthEst(spec[:, 2], lv, flag, interp)
        assert isinstance(one, float) and one == want[2]
    _, _, want, _ = wr.width(a.astype(np.float32), -6.0, 1, 4)
    np.testing.assert_array_equal(rsp.ampConstrWidthEst(a, -6.0, 1, 4), want)
    assert wd.ampConstrWidthEst(np.zeros(16), -6.0, 1, 4) == 0.0


@pytest.fixture(scope="module")
def dmx():
    import torch
    from rsp.dmx import DmxFrameProcessor
    echo = np.load(os.path.join(GOLDEN, "dmx_32x512.npz"))["echo"].astype(np.complex64)
    P, R = echo.shape
    proc = DmxFrameProcessor(freInd=2, P=P, R=R)
    e = np.stack([np.stack([echo, 0.7 * echo]), np.stack([echo[::-1], 0.6 * echo[::-1]])]).astype(np.complex64)
    yield proc, torch.from_numpy(e).cuda()
    proc.close()


@pytest.mark.parametrize("condense", [None, dict(gap=(1, 1))], ids=["hits", "plots"])
def test_dmx_frame_processor_width(dmx, condense):
    """process_dev(width=...) on the dmx_32x512 golden-sized input: the spans are the restatement's
    on the planes the processor returns, widthDots is the span gathered through the measurement's
    cells, and width=None leaves the dict as it was."""
    import torch
    proc, echo = dmx
    base = proc.process_dev(echo, 4, condense=condense)
    out = proc.process_dev(echo, 4, condense=condense, width=dict(amp_constr=-6.0, interp=4))
    torch.cuda.synchronize()
    pairs = [(p, k) for p in ("short", "long") for k in ("flag", "flagV")]
    assert set(out) == set(base) | {(p, k, w) for p, k in pairs for w in ("width", "widthDots")}
    if condense is None:
        assert len(base) == 8
    for k in base:
        if not isinstance(base[k], tuple):
            assert torch.equal(base[k], out[k]), k
            continue
        # (est, cells, count) or (plots, count): the lists are written up to their counts
        a, b = [t.cpu().numpy() for t in base[k]], [t.cpu().numpy() for t in out[k]]
        np.testing.assert_array_equal(a[-1], b[-1])
        for x, y in zip(a[:-1], b[:-1]):
            for cpi in range(x.shape[0]):
                m = min(int(a[-1][cpi, 0]), x.shape[1])
                assert x[cpi, :m].tobytes() == y[cpi, :m].tobytes(), k
    ps = proc.spec.cfar_segments[0][1]
    amp = out["sum"].cpu().numpy()
    tested = ties = hits = 0
    for part, (lo, hi) in (("short", (0, ps)), ("long", (ps, proc.spec.R_out))):
        for kind, plane in (("flag", "peak" if condense else "flag"), ("flagV", "peakV" if condense else "flagV")):
            f = out[plane].cpu().numpy()
            span, count = (t.cpu().numpy() for t in out[(part, kind, "width")])
            _, cells, n = (t.cpu().numpy() for t in out[(part, kind)])
            w = out[(part, kind, "widthDots")].cpu().numpy()
            assert w.dtype == np.float64 and w.shape == cells.shape[:2]
            for b in range(amp.shape[0]):
                t, k = wr.compare(span[b], count[b], amp[b][:, lo:hi], f[b][:, lo:hi].any(axis=0), -6.0, 4, True)
                tested, ties = tested + t, ties + k
                m = min(int(n[b, 0]), cells.shape[1])
                hits += m
                col = cells[b, :m, 1]
                np.testing.assert_array_equal(w[b, :m], (span[b, col, 1] - span[b, col, 0]) / 4.0)
                assert np.isnan(w[b, m:]).all()
                assert (span[b, col] >= 0).all()            # a measured hit's column is a computed one
    _check(tested, ties)
    assert hits > 0
    with pytest.raises(TypeError):
        proc.process_dev(echo, 4, condense=condense, width=dict(amp_constr=-6.0, interp=4, level=3))
