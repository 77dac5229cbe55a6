"""Every MTD kernel instance against an fp64 slow-time DFT, row by row and column by column.

launch_mtd picks a kernel from the Doppler length, the beam count and the Doppler CFAR window: one
of fourteen radix instances on one beam (MtdCfg: tiles of W range bins by T threads), three on two
beams, six Bluestein transform lengths, each without CFAR, with the compiled 5 + 7 Doppler window
or with a runtime window.  tests/mtd_ref.py holds the sweep's table, its scenes and the fp64
restatement they are compared with; tests/test_mtd_ref_cpu.py pins those without a GPU.  The tile
each case must run on (TILE, TILE2, BLUESTEIN below) is written by hand from MtdCfg's rules and
compared with what rsp_cfar_plan reports.

Every case feeds Engine.mtd_dev three CPIs of designed pulse-compressed rows -- noise, tones,
impulses -- so the CPI strides (cpi * pin * beams rows in, cpi * V * R cells out) are always in
play, three times: without CFAR, with the 5 + 7 window and with a 3 + 2 window (where the band
holds them: mtd_ref.cfar_windows).  Every output lies between guard planes of 0xA5 bytes.

Bars, against mtd_ref of the complex64 values widened to complex128 (RDM_TOL = MAX_TOL = 1e-5):
every CPI's plane in both figures; on the noise CPI every row and every column as a relative
Frobenius error (an fp32 radix FFT's rms error is of order eps * log2 V = 6e-8 * 11 ~ 7e-7 at
V = 2048, Bluestein three such transforms and fp32 chirp tables: 1e-5 leaves about a factor of
five at worst; with an MTI, whose nulls leave rows of almost no energy, a row is measured against
the median row where it is smaller: rows_cols); rows of the zero band == 0.0 and no other noise
row 0; every tone's argmax on its
declared row; every impulse cell within 1e-5 of |a| w[p] (with an MTI: of the column's largest
reference cell); flags against the C oracle fed the GPU's own RDM, no mismatch outside its
near-threshold mask (capped on the CPU).  One line per case records the worst figures.
"""
import dataclasses

import numpy as np
import pytest

import mtd_ref as mr
from _util import MAX_TOL, NEAR_TOL, RDM_TOL, flag_mismatch, max_rel, oracle_flags_c, rel_err
from test_gpu_cfar_dispatch import cfar_obj, check_guards, guarded

pytestmark = pytest.mark.gpu

BATCH = 3
# One beam, radix: V -> (W range bins, T threads).  E = 16 rows per thread (24 for 3 * 2^k), G = V / E
# threads per range bin; T = 256, but for a power of two from 512 on 16 * G, at most 1024; W = T / G.
TILE = {16: (256, 256), 32: (128, 256), 48: (128, 256), 64: (64, 256), 96: (64, 256), 128: (32, 256),
        192: (32, 256), 256: (16, 256), 384: (16, 256), 512: (16, 512), 768: (8, 256), 1024: (16, 1024),
        1536: (4, 256), 2048: (8, 1024)}
# Two beams: always 256 threads.
TILE2 = {512: (8, 256), 1024: (4, 256), 2048: (2, 256)}
# Bluestein: P -> NF, the smallest power of two >= 2 P - 1 (at least 64); the tile is TILE[NF].
BLUESTEIN = {2: 64, 17: 64, 31: 64, 33: 128, 63: 128, 65: 256, 127: 256, 129: 512, 255: 512, 257: 1024, 511: 1024,
             513: 2048, 1023: 2048}


def expected_tile(case):
    """(W, T, Bluestein NF or 0) by the tables above."""
    if case.beams == 2:
        return TILE2[case.V] + (0,)
    if case.V in TILE:
        return TILE[case.V] + (0,)
    nf = BLUESTEIN[case.V]
    return TILE[nf] + (nf,)


def case_spec(pin, R, window=mr.KAISER, shift=1, zdiv=0, zends=0, nfft=0, beams=1):
    """A context whose pulse compression is one matched-filter segment over the whole row (the MTD
    tests feed rows directly; the two-beam difference and the window stream run it)."""
    from test_gpu_pc_geometry import MF, seg_spec
    spec = seg_spec(R, R, [(MF, 0, R, 0, R, 512 if R <= 512 else 1024, 67)])(pin)
    return dataclasses.replace(spec, window=window, fftshift=shift, zero_v_div=zdiv, mtd_nfft=nfft, beams=beams,
                               zero_ends=zends)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def rows_cols(got, want, zb, mti=False):
    """Worst relative Frobenius error over the unzeroed rows, and over the columns (of those rows).
    mti: a row is measured against the median row's norm where its own is smaller.  The MTI
    x[p + lag] - x[p] nulls the bins with k lag = 0 (mod V): at lag 1 the DC row of 768 noise
    pulses has 0.005 of the median row's norm, while an FFT's rounding error in a bin goes with the
    column's rms, not with the bin's own value -- the same transform in complex64 on the CPU is
    1.3e-5 off on that row.  Without an MTI every noise row stands alone."""
    d, w = (got.astype(np.float64) - want)[~zb], want[~zb]
    rn = np.linalg.norm(w, axis=1)
    if mti:
        rn = np.maximum(rn, np.median(rn))
    return (float(np.max(np.linalg.norm(d, axis=1) / rn)),
            float(np.max(np.linalg.norm(d, axis=0) / np.linalg.norm(w, axis=0))))


def check_rdm(what, rdm, want, zb, tone_rows, imp, lag, w):
    """The RDM bars of the module docstring on [3, V, R]; returns (plane, max, row, column) figures."""
    assert np.isfinite(rdm).all(), what
    assert (rdm[:, zb] == 0.0).all(), what + ": a row of the zero band is not exactly 0"
    assert not (rdm[0][~zb] == 0.0).any(), what + ": a zero outside the band"
    plane = max(rel_err(rdm[b], want[b]) for b in range(BATCH))
    peak = max(max_rel(rdm[b], want[b]) for b in range(BATCH))
    row, col = rows_cols(rdm[0], want[0], zb, mti=lag > 0)
    print("%s: plane %.2e max %.2e noise row %.2e col %.2e" % (what, plane, peak, row, col))
    assert plane < RDM_TOL and peak < MAX_TOL, (what, plane, peak)
    assert row < RDM_TOL and col < RDM_TOL, (what, row, col)
    ok = mr.peaked_columns(want[1], tone_rows, zb)
    arg = rdm[1].argmax(axis=0)
    assert (arg[ok] == tone_rows[ok]).all(), (what, "tones", np.flatnonzero(ok & (arg != tone_rows))[:8])
    p, a = imp
    scale = want[2][~zb].max(axis=0)
    dev = np.abs(rdm[2].astype(np.float64) - want[2])[~zb]
    assert (dev <= 1e-5 * scale[None, :]).all(), (what, "impulses", np.flatnonzero((dev > 1e-5 * scale).any(axis=0))[:8])
    if not lag and w is not None:
        flat = np.abs(a) * w[p]
        assert (np.abs(rdm[2].astype(np.float64)[~zb] - flat[None, :]) <= 1e-5 * flat[None, :]).all(), (what, "|a| w[p]")
    return plane, peak, row, col


def check_flags(what, flag, fv, rdm, cf):
    """Flags of every CPI against the oracle fed the RDM the same call returned."""
    assert flag.max() <= 1 and fv.max() <= 1, what + ": a flag byte that is neither 0 nor 1"
    oflag, oflagV, amb = oracle_flags_c(rdm.astype(np.float64), cf, NEAR_TOL)
    hard, soft = flag_mismatch(flag, oflag, amb)
    hardv, softv = flag_mismatch(fv, oflagV, amb)
    print("%s: flags %d / %d Doppler hits (noise CPI %d / %d), mask %d, mismatches hard %d+%d soft %d+%d"
          % (what, int(oflag.sum()), int(oflagV.sum()), int(oflag[0].sum()), int(oflagV[0].sum()), int(amb.sum()),
             hard, hardv, soft, softv))
    assert hard == 0 and hardv == 0, (what, hard, hardv)
    assert soft <= int(amb.sum()) and softv <= int(amb.sum()), (what, soft, softv)
    assert oflagV[0].sum() >= 1, what


def run_mtd(torch, call, shape, cf, diff=False):
    """call(rdm=, flag=, flagV=, cfar=[, diff=]) into guarded buffers -> numpy outputs."""
    bufs = {"rdm": guarded(torch, shape, torch.float32)}
    if diff:
        bufs["diff"] = guarded(torch, shape, torch.float32)
    if cf is not None:
        bufs["flag"] = guarded(torch, shape, torch.uint8)
        bufs["flagV"] = guarded(torch, shape, torch.uint8)
    call(cfar=cf, **{k: v[1] for k, v in bufs.items()})
    torch.cuda.synchronize()
    out = {}
    for k, (raw, _) in bufs.items():
        if k in ("rdm", "diff"):
            out[k] = check_guards(raw, shape, 4).view(np.float32).reshape(shape)
        else:
            out[k] = check_guards(raw, shape).reshape(shape)
    return out


def references(case, x):
    zb = case.band()
    want = []
    for b in range(BATCH):
        o = mr.mtd_ref(x[b].astype(np.complex128), case.w(), case.V, case.shift, zb, case.lag, case.beams)
        want.append(o[0] if case.beams == 2 else o)
    return zb, np.stack(want)


@pytest.mark.parametrize("case", mr.CASES, ids=lambda c: c.id)
def test_instance(torch_cuda, case):
    torch = torch_cuda
    from rsp.engine import Engine
    W, T, nf = expected_tile(case)
    assert case.G == T // W
    assert case.R == 2 * W + 5 or (case.R // W in (32, 64) and case.R % W == 0 and W < 32)
    x, tone_rows, imp = mr.cpis(case)
    zb, want = references(case, x)
    d_pc = torch.from_numpy(x).cuda()
    shape = (BATCH, case.V, case.R)
    eng = Engine(case_spec(case.pin, case.R, case.window, case.shift, case.zdiv, case.zends, case.nfft, case.beams),
                 device=0)
    try:
        if case.lag:
            eng.set_prefilter(mti_lag=case.lag)
        w = case.w() if case.beams == 1 else None
        worst = np.zeros(4)
        runs = [("nocfar", None)] + [(name, cfar_obj(win, mr.CFAR_T, 0, case.cfar_zdiv, [], case.methods))
                                     for name, win in mr.cfar_windows(case)]
        if len(runs) == 1 and case.V >= 11:      # a flat plane runs no CFAR; its tile is reported all the same
            plan = eng.cfar_plan(cfar_obj(mr.W32 + mr.W32, mr.CFAR_T, 0, 0, [], (0, 0)), BATCH)
            assert (plan["tile_w"], plan["threads"], plan["bluestein"], plan["window_compiled"]) == (W, T, nf, 0)
        for name, cf in runs:
            what = "%s %s" % (case.id, name)
            if cf is not None:
                plan = eng.cfar_plan(cf, BATCH)
                got = (plan["tile_w"], plan["threads"], plan["bluestein"], plan["window_compiled"])
                assert got == (W, T, nf, int(name == "w57" and nf == 0)), (what, got)
            out = run_mtd(torch, lambda **kw: eng.mtd_dev(d_pc, **kw), shape, cf)
            worst = np.maximum(worst, check_rdm(what, out["rdm"], want, zb, tone_rows, imp, case.lag, w))
            if cf is not None:
                check_flags(what, out["flag"], out["flagV"], out["rdm"], cf)
        print("MTD-INST %-18s pin %4d V %4d R %4d beams %d W %3d T %4d nf %4d runs %d: plane %.2e max %.2e row %.2e col %.2e"
              % ((case.id, case.pin, case.V, case.R, case.beams, W, T, nf, len(runs)) + tuple(worst)))
    finally:
        eng.close()


def test_bluestein_rejects_1025(torch_cuda):
    """2 * 1025 - 1 points do not fit the largest transform (2048) and 1025 has no radix plan."""
    from rsp import RspError
    from rsp.engine import Engine
    with pytest.raises(RspError) as ei:
        Engine(case_spec(1025, 21), device=0)
    assert ei.value.code == 3      # RSP_ERR_UNSUPPORTED
    Engine(case_spec(1025, 21, nfft=2048), device=0).close()      # zero-padded to 2048 it is built


def _echo(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@pytest.mark.parametrize("case", [c for c in mr.CASES if c.beams == 2], ids=lambda c: c.id)
def test_two_beam_difference(torch_cuda, case):
    """The difference plane |X_R| - |X_L| leaves only the whole chain: pulse compression alone gives
    the rows the MTD reads, mtd_ref of those the planes the chain must return.  Bar of the
    difference: the sum of the two magnitudes' own bars, 1e-5 (||L||_F + ||R||_F)."""
    torch = torch_cuda
    from rsp.engine import Engine
    pin, V, R = case.pin, case.V, case.R
    echo = torch.from_numpy(_echo((BATCH, 2, pin, R), mr.SEED + 7)).cuda()
    eng = Engine(case_spec(pin, R, case.window, case.shift, case.zdiv, case.zends, case.nfft, 2), device=0)
    try:
        d_pc = torch.empty((BATCH * 2, pin, R), dtype=torch.complex64, device="cuda")
        eng.pc_dev(echo.view(BATCH * 2, pin, R), d_pc)
        torch.cuda.synchronize()
        pc = d_pc.cpu().numpy().reshape(BATCH, 2, pin, R).astype(np.complex128)
        assert np.isfinite(pc).all() and pc.any()
        shape = (BATCH, V, R)
        out = run_mtd(torch, lambda **kw: eng.run_dev(echo, **kw), shape, None, diff=True)
        zb = case.band()
        worst = 0.0
        for b in range(BATCH):
            s, d = mr.mtd_ref(pc[b], case.w(), V, case.shift, zb, 0, 2)
            left, right = mr.beam_magnitudes(pc[b], case.w(), V, case.shift)
            assert (out["rdm"][b][zb] == 0.0).all() and not (out["rdm"][b][~zb] == 0.0).any()
            es = rel_err(out["rdm"][b], s)
            ed = float(np.linalg.norm(out["diff"][b].astype(np.float64) - d) / (np.linalg.norm(left) + np.linalg.norm(right)))
            row, col = rows_cols(out["rdm"][b], s, zb)
            # the difference is not zeroed, and |R| - |L| changes sign across the plane
            assert (out["diff"][b] > 0).any() and (out["diff"][b] < 0).any()
            big = np.abs(d) > 1e-3 * np.abs(d).max()
            assert np.array_equal(np.sign(out["diff"][b][big]), np.sign(d[big]))
            worst = max(worst, es, ed, row, col)
            assert es < RDM_TOL and ed <= 1e-5 and row < RDM_TOL and col < RDM_TOL, (case.id, b, es, ed, row, col)
        print("MTD-INST %-18s difference plane through the chain: worst of sum, difference, row, column %.2e"
              % (case.id, worst))
    finally:
        eng.close()


@pytest.mark.parametrize("P,W,G,win", mr.WINDOW_CASES, ids=["p%d-win%d" % (c[0], c[3]) for c in mr.WINDOW_CASES])
def test_window_stream(torch_cuda, P, W, G, win):
    """The sliding-window stream (nwin, win_start) against mtd_ref of the CPU-sliced pulse-compressed
    rows: window i of frame pair (n, n + 1) is rows [floor(i P / win + 0.5), +P) of the two frames."""
    torch = torch_cuda
    from rsp.engine import Engine
    assert TILE[P] == (W, G * W)
    R, nfr = 2 * W + 5, 2
    window = (mr.HAMMING, mr.KAISER)[win % 2]
    frames = torch.from_numpy(_echo((1, nfr + 1, P, R), mr.SEED + 11 + win)).cuda()
    eng = Engine(case_spec(P, R, window, 1, 150), device=0)
    try:
        d_pc = torch.empty((nfr + 1, P, R), dtype=torch.complex64, device="cuda")
        eng.pc_dev(frames.view(nfr + 1, P, R), d_pc)
        torch.cuda.synchronize()
        pc = d_pc.cpu().numpy().astype(np.complex128)
        zb = mr.zero_band(P, zero_v_div=150)
        w = mr.slow_time_window(window, P)
        starts = mr.window_starts(P, win)
        assert starts[0] == 0 and len(set(starts)) == win and max(starts) < P
        want = np.stack([mr.mtd_ref(np.concatenate([pc[n], pc[n + 1]])[s:s + P], w, P, 1, zb)
                         for n in range(nfr) for s in starts])
        cf = cfar_obj(mr.W57 + mr.W57, mr.CFAR_T, 0, 20, [], (0, 0))
        shape = (nfr * win, P, R)

        def call(cfar, **bufs):
            eng.window_dev(frames, win, cfar=cfar, **{k: v.view(1, nfr, win, P, R) for k, v in bufs.items()})

        out = run_mtd(torch, call, shape, cf)
        rdm = out["rdm"]
        assert (rdm[:, zb] == 0.0).all() and not (rdm[:, ~zb] == 0.0).any()
        worst = np.zeros(4)
        for i in range(nfr * win):
            fig = (rel_err(rdm[i], want[i]), max_rel(rdm[i], want[i])) + rows_cols(rdm[i], want[i], zb)
            worst = np.maximum(worst, fig)
            assert max(fig) < RDM_TOL, (P, win, i, fig)
        check_flags("window P %d win %d" % (P, win), out["flag"], out["flagV"], rdm, cf)
        print("MTD-INST window-p%d-win%-2d   R %4d W %3d: plane %.2e max %.2e row %.2e col %.2e"
              % ((P, win, R, W) + tuple(worst)))
    finally:
        eng.close()
