"""process_dev(integrate=...) of the DMX frame processor at a small DMX-shaped preset (P = 32, the
dmx_32x512 golden's geometry) against the same stages composed by hand: run_dev(cfar=None) -> sum_dev per
part and plane -> cfar_dev -> measure_dev, byte for byte; the same with m, with detector=, and with
condense= + track=; integrate=None against a call without the argument; two half batches against one
whole; reset_integration().
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the frame time of the full waveform (1536 PRTs), so that the fast rows of this small preset walk too
INTEG = dict(n=3, dt=1536 * 52.08e-6)
MAX_HITS = 512
# 32 pulses in a 2048-point Doppler transform: a line is 64 rows wide, far wider than the CFAR window, so
# the cell-averaging CFAR flags nothing on this input; the ordered-statistic detector near the 7th
# smallest neighbour does, and the tests that need hits take their flags from it
DET = dict(k=(7, 7), union=(True, True), T=(1.25, 1.25))


@pytest.fixture(scope="module")
def dmx():
    import torch
    from rsp.dmx import DmxFrameProcessor
    echo = np.load(os.path.join(GOLDEN, "dmx_32x512.npz"))["echo"].astype(np.complex64)
    P, R = echo.shape
    proc = DmxFrameProcessor(freInd=2, P=P, R=R)
    e = np.stack([np.stack([echo, 0.7 * echo]), np.stack([echo[::-1], 0.6 * echo[::-1]]),
                  np.stack([0.8 * echo, echo[::-1]]), np.stack([echo, 0.9 * echo])]).astype(np.complex64)
    yield proc, torch.from_numpy(e).cuda()
    proc.close()


def _same_out(got, want, keys=None):
    """Planes byte for byte; (est, cells, count)-like tuples: the counts, and every row up to its count."""
    import torch
    for k in (want if keys is None else keys):
        a, b = got[k], want[k]
        if not isinstance(b, tuple):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), k
            continue
        a, b = [t.cpu().numpy() for t in a if t is not None], [t.cpu().numpy() for t in b if t is not None]
        if len(k) == 3 and k[2] == "tracks":
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes(), k
            continue
        np.testing.assert_array_equal(a[-1], b[-1])
        for x, y in zip(a[:-1], b[:-1]):
            for cpi in range(x.shape[0]):
                m = min(int(b[-1][cpi, 0]), x.shape[1])
                assert x[cpi, :m].tobytes() == y[cpi, :m].tobytes(), k


def _by_hand(proc, echo, beam, integ, detector=None, m=None, spread=0):
    """The integrate path from its parts, on Integrators of its own."""
    import torch
    from rsp.integrate import Integrator, walk_shifts
    from rsp.oscfar import OsCfar
    B = echo.shape[0]
    shp = (B, proc.spec.V, proc.spec.R_out)
    out = {k: torch.empty(shp, dtype=t, device=echo.device) for k, t in
           (("sum_cpi", torch.float32), ("diff_cpi", torch.float32), ("sum", torch.float32), ("diff", torch.float32),
            ("flag", torch.uint8), ("flagV", torch.uint8))}
    proc.eng.run_dev(echo, rdm=out["sum_cpi"], diff=out["diff_cpi"], cfar=None)
    rS, rL, vS, dR, dV = proc.scales
    n = integ["n"]
    shift = walk_shifts(vS, integ["dt"], dR, n, 1.0)
    ps = proc.spec.cfar_segments[0][1]
    parts = (("short", (0, ps), rS), ("long", (ps, proc.spec.R_out), rL))
    made = []
    for plane in ("sum", "diff"):
        for _, cols, _ in parts:
            it = Integrator(0, n=n)
            made.append(it)
            it.sum_dev(out[plane + "_cpi"], shift=shift, cols=cols, out=out[plane])
    if detector is None:
        proc.eng.cfar_dev(out["sum"], out["flag"], flagV=out["flagV"], cfar=proc.cfar)
    else:
        import dataclasses
        cf = dataclasses.replace(proc.cfar, TV=float(detector["T"][0]), TR=float(detector["T"][1]))
        OsCfar(engine=proc.eng).detect_dev(out["sum"], cf, detector["k"], detector["union"], flag=out["flag"],
                                          flagV=out["flagV"])
    if m is not None:
        for fk in ("flag", "flagV"):
            raw, out[fk] = out[fk], torch.empty_like(out[fk])
            out[fk + "_cpi"] = raw
            for _, cols, _ in parts:
                it = Integrator(0, n=n, m=m, spread=spread)
                made.append(it)
                it.count_dev(raw, shift=shift, cols=cols, out=out[fk])
    o = proc.o
    p = proc.meas.params(o["extraDots"], dR, o["rInterpTimes"], dV, o["vInterpTimes"],
                         float(proc.kValues[proc.freInd, beam]), beam, o["beamAngleStep"], o["eleAngleComp"],
                         o["eleAngleSysErr"], proc.spec.radar["M0"])
    for fk in ("flag", "flagV"):
        for part, cols, rs in parts:
            out[(part, fk)] = proc.meas.measure_dev(out["sum"], out["diff"], out[fk], p, rs, vS, max_hits=MAX_HITS,
                                                    cols=cols)
    torch.cuda.synchronize()
    for it in made:
        it.close()
    return out, shift


def test_integrate_equals_the_hand_composition(dmx):
    import torch
    proc, echo = dmx
    proc.reset_integration()
    out = proc.process_dev(echo, 3, max_hits=MAX_HITS, integrate=INTEG)
    want, shift = _by_hand(proc, echo, 3, INTEG)
    torch.cuda.synchronize()
    assert np.abs(shift).max() >= 2 and (shift == 0).any()     # some rows walk, some do not
    assert set(out) == set(want)
    _same_out(out, want)
    # the per-CPI planes are the plain call's, and the integration changed something
    base = proc.process_dev(echo, 3, max_hits=MAX_HITS)
    _same_out(dict(sum=out["sum_cpi"], diff=out["diff_cpi"]), base, keys=("sum", "diff"))
    assert torch.equal(out["sum"][0], base["sum"][0]) and not torch.equal(out["sum"][1], base["sum"][1])
    with pytest.raises(TypeError):
        proc.process_dev(echo, 3, integrate=dict(n=3, walks=True))


def test_integrate_none_changes_nothing(dmx):
    proc, echo = dmx
    a = proc.process_dev(echo, 3, max_hits=MAX_HITS)
    b = proc.process_dev(echo, 3, max_hits=MAX_HITS, integrate=None)
    assert set(a) == set(b)
    _same_out(b, a)


def test_integrate_with_m(dmx):
    import torch
    proc, echo = dmx
    proc.reset_integration()
    out = proc.process_dev(echo, 3, max_hits=MAX_HITS, integrate=dict(INTEG, m=2, spread=1), detector=DET)
    want, _ = _by_hand(proc, echo, 3, INTEG, detector=DET, m=2, spread=1)
    assert set(out) == set(want)
    _same_out(out, want)
    assert not out["flag"][0].any()                # strict: nothing before the second CPI
    assert out["flag_cpi"].any() and out["flag"].any()
    assert not torch.equal(out["flag"], out["flag_cpi"])
    # the cell-averaging CFAR in front of the count: the same composition
    proc.reset_integration()
    out = proc.process_dev(echo, 3, max_hits=MAX_HITS, integrate=dict(INTEG, m=2, spread=1))
    want, _ = _by_hand(proc, echo, 3, INTEG, m=2, spread=1)
    _same_out(out, want)


def test_integrate_with_detector(dmx):
    proc, echo = dmx
    proc.reset_integration()
    out = proc.process_dev(echo, 3, max_hits=MAX_HITS, integrate=INTEG, detector=DET)
    want, _ = _by_hand(proc, echo, 3, INTEG, detector=DET)
    assert set(out) == set(want)
    _same_out(out, want)
    assert out["flag"].any() and int(out[("long", "flag")][2][:, 0].sum()) > 0


def test_integrate_with_condense_and_track(dmx):
    import torch
    from rsp.condense import Condense
    from rsp.track import Tracker
    proc, echo = dmx
    track = dict(gate=(60.0, 3.0), alpha=(0.5, 0.5, 0.25), confirm=(2, 3), drop=(2, 3), max_tracks=64)
    proc.reset_integration()
    proc.reset_tracks()
    out = proc.process_dev(echo, 3, max_hits=MAX_HITS, integrate=INTEG, condense=dict(gap=(1, 1)), track=track,
                           detector=DET)
    want, _ = _by_hand(proc, echo, 3, INTEG, detector=DET)
    _same_out(out, want, keys=("sum", "diff", "sum_cpi", "diff_cpi", "flag", "flagV"))
    # condense, measure and track by hand on the integrated planes
    cond = Condense(0)
    trk = Tracker(0, slots=4, dt=proc.spec.P / proc.spec.radar["prf"], **track)
    try:
        rS, rL, vS, dR, dV = proc.scales
        o = proc.o
        p = proc.meas.params(o["extraDots"], dR, o["rInterpTimes"], dV, o["vInterpTimes"],
                             float(proc.kValues[proc.freInd, 3]), 3, o["beamAngleStep"], o["eleAngleComp"],
                             o["eleAngleSysErr"], proc.spec.radar["M0"])
        ps = proc.spec.cfar_segments[0][1]
        hand = {}
        for fk, pk in (("flag", "peak"), ("flagV", "peakV")):
            hand[pk] = torch.empty_like(want[fk])
            for part, cols, rs in (("short", (0, ps), rS), ("long", (ps, proc.spec.R_out), rL)):
                _, plots, count = cond.condense_dev(want["sum"], want[fk], gap=(1, 1), wrap_v=False, max_plots=MAX_HITS,
                                                    cols=cols, peak=hand[pk])
                hand[(part, fk, "plots")] = (plots, count)
                hand[(part, fk)] = proc.meas.measure_dev(want["sum"], want["diff"], hand[pk], p, rs, vS,
                                                         max_hits=MAX_HITS, cols=cols)
        for (part, fk), slot in proc.TRACK_SLOTS.items():
            est, _, count = hand[(part, fk)]
            hand[(part, fk, "tracks")] = trk.update_dev(est, count, slot=slot)
        torch.cuda.synchronize()
        _same_out(out, hand)
        assert sum(int(hand[(part, "flag", "plots")][1][:, 0].sum()) for part in ("short", "long")) > 0
    finally:
        cond.close()
        trk.close()
        proc.reset_tracks()


def test_two_half_batches_equal_one_whole_and_reset(dmx):
    import torch
    proc, echo = dmx
    kw = dict(max_hits=MAX_HITS, integrate=dict(INTEG, m=2), detector=DET)
    proc.reset_integration()
    whole = proc.process_dev(echo, 3, **kw)
    proc.reset_integration()
    h1 = proc.process_dev(echo[:2], 3, **kw)
    h2 = proc.process_dev(echo[2:], 3, **kw)
    torch.cuda.synchronize()
    assert set(h1) == set(whole)
    for k in whole:
        if not isinstance(whole[k], tuple):
            assert torch.equal(torch.cat([h1[k], h2[k]]), whole[k]), k
        else:
            _same_out({k: tuple(torch.cat([a, b]) for a, b in zip(h1[k], h2[k]))}, whole, keys=(k,))
    # without a reset the next call continues the dwell; after one it is the first call again
    cont = proc.process_dev(echo, 3, **kw)
    assert not torch.equal(cont["sum"][0], whole["sum"][0])
    proc.reset_integration()
    again = proc.process_dev(echo, 3, **kw)
    _same_out(again, whole)
