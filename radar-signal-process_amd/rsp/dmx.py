"""The DMX per-frame processing loop on the GPU (SURVEY.md rows a4/a8 + §8f-3): what
MatlabProcess_xuzerui/CFAR_WangCai/DMX_SignalProcessing_main_xzr.m does for one frame of the
two-beam long/short-pulse waveform (flag_Mode 1), from the left/right echo matrices to the
per-part target series:

  * scales (:93-96, :313-327): deltaR = c*ts/2, fc = freValueGen(freInd), rScale_short /
    rScale_long with the range calibration of :250-253, deltaV, fScale = fftshift(...), vScale;
  * pulse compression, 2048-point Doppler, |L|+|R| / |R|-|L|, zeroSetFlagMTD and executeCFAR on
    each part (:331-472): Engine(presets.dmx_native(fc=...)).run_dev -> sum, diff, flag, flagV;
  * motionParaMeasure on the short and the long part, for flag and for flagV (:489-516):
    Measure.measure_dev over the column windows of the same device planes.

Frames are batched ([batch][2 beams][P][R] complex64 on the device); everything between the
echo and the estimates stays in HBM.  The frame reader the main calls at :307, frameDataRead_A,
is MatlabProcess_xuzerui/Show_Read.m (two arguments, with the in-file frame seek) and
frameDataRead_A_xzr.m (three arguments, the seek commented out); both are written for the
legacy waveform's point_PRT = 1031.  No reader for this waveform's point_PRT = 566 (:111) ships
in the reference: process_records_dev ASSUMES the same record layout with point_prt = 566
(28-byte head, 12 bytes per sample, 8-byte tail) and decodes it on the GPU (rsp.ingest.LegacyIngest);
process_dev takes the echo matrices themselves.
"""
import math

import numpy as np

from . import presets
from .engine import Engine
from .measure import Measure, angle_KvalueGen, freValueGen

# DMX_SignalProcessing_main_xzr.m:250-270
DMX_DEFAULTS = dict(rSysErr_short=0.0, rSysErr_long=62.0 * 12.0, rMeasureErr_short=297.0, rMeasureErr_long=92.0,
                    extraDots=2, rInterpTimes=8, vInterpTimes=4, eleAngleComp=0.0, eleAngleSysErr=0.0,
                    beamAngleStep=5.0, sysNum=1, northAngle=29.01, angleE1=5.9)


def dmx_scales(spec, freInd, **kw):
    """(rScale_short, rScale_long, vScale, deltaR, deltaV) of :93-96 and :313-327."""
    o = dict(DMX_DEFAULTS, **kw)
    fs, prf = spec.radar["fs"], spec.radar["prf"]
    deltaR = presets.C_LIGHT * (1.0 / fs) / 2.0
    lamda = presets.C_LIGHT / freValueGen(freInd)
    point_short = spec.cfar_segments[0][1]
    fft_num = spec.R_out - point_short
    N = spec.V
    rScale_short = np.arange(point_short) * deltaR + o["rSysErr_short"] - o["rMeasureErr_short"]
    rScale_long = np.arange(fft_num) * deltaR + o["rSysErr_long"] - o["rMeasureErr_long"]
    deltaDoppler = prf / N
    deltaV = lamda * deltaDoppler / 2.0
    fScale = np.fft.fftshift(np.arange(-N // 2, N // 2) * deltaDoppler)
    vScale = -lamda * fScale / 2.0
    return rScale_short, rScale_long, vScale, deltaR, deltaV


class DmxFrameProcessor:
    """One frequency number's DMX chain + measurement on one GPU."""

    def __init__(self, freInd=0, device=0, P=1536, R=566, **kw):
        self.o = dict(DMX_DEFAULTS, **kw)
        self.freInd = int(freInd)
        self.spec = presets.dmx_native(P=P, R=R, fc=freValueGen(self.freInd))
        self.cfar = presets.default_cfar(self.spec)
        self.eng = Engine(self.spec, device=device)
        self.meas = Measure(device)
        self.kValues = angle_KvalueGen(self.o["sysNum"])
        self.scales = dmx_scales(self.spec, self.freInd, **kw)
        self.device = self.meas.device
        self._ingest = None
        self._cond = None
        self._width = None
        self._tracker = None
        self._track_opts = None
        self._os = None
        self._integ = {}
        self._integ_opts = None

    def close(self):
        self.eng.close()
        self.meas.close()
        if self._tracker is not None:
            self._tracker.close()
        if self._cond is not None:
            self._cond.close()
        if self._width is not None:
            self._width.close()
        if self._ingest is not None:
            self._ingest.close()

    # the tracker's slot of each (part, kind)
    TRACK_SLOTS = {("short", "flag"): 0, ("long", "flag"): 1, ("short", "flagV"): 2, ("long", "flagV"): 3}

    def reset_tracks(self):
        """Forget every track of process_dev(track=...)."""
        if self._tracker is not None:
            self._tracker.reset()

    def _track_options(self, track):
        """track=dict(...) as the Tracker's keyword arguments; dt defaults to the frame time P / prf."""
        track = dict(track)
        opts = dict(gate=tuple(track.pop("gate")) if "gate" in track else None,
                    alpha=tuple(track.pop("alpha", (0.5, 0.5, 0.5))), confirm=tuple(track.pop("confirm", (3, 5))),
                    drop=tuple(track.pop("drop", (2, 4))), max_tracks=int(track.pop("max_tracks", 256)),
                    dt=float(track.pop("dt", self.spec.P / self.spec.radar["prf"])),
                    rate_sign=float(track.pop("rate_sign", 1.0)))
        if track:
            raise TypeError("process_dev: track takes gate, alpha, confirm, drop, max_tracks, dt and rate_sign, not %s"
                            % sorted(track))
        if opts["gate"] is None:
            raise TypeError("process_dev: track needs gate=(gate_r, gate_v)")
        return opts

    def _tracks(self, out, opts, with_flagV):
        """out[(part, kind, 'tracks')] of every measured (part, kind), each on its own slot."""
        from .track import Tracker
        if self._tracker is None or opts != self._track_opts:
            if self._tracker is not None:
                self._tracker.close()
            self._tracker = Tracker(self.device.index or 0, slots=len(self.TRACK_SLOTS), **opts)
            self._track_opts = opts
        for (part, fk), slot in self.TRACK_SLOTS.items():
            if fk == "flagV" and not with_flagV:
                continue
            est, _, count = out[(part, fk)]
            out[(part, fk, "tracks")] = self._tracker.update_dev(est, count, slot=slot)
        return out

    def reset_integration(self):
        """Forget the CPIs of process_dev(integrate=...): the next call starts every ring anew."""
        for integ in self._integ.values():
            integ.reset()

    def _integrate_options(self, integrate):
        """integrate=dict(...) as (n, shift, m, spread): shift the int32 [n-1][V] walk table, or None."""
        from .integrate import walk_shifts
        integrate = dict(integrate)
        n = int(integrate.pop("n", 4))
        walk = bool(integrate.pop("walk", True))
        rate_sign = float(integrate.pop("rate_sign", 1.0))
        dt = float(integrate.pop("dt", self.spec.P / self.spec.radar["prf"]))
        m = integrate.pop("m", None)
        spread = int(integrate.pop("spread", 0))
        if integrate:
            raise TypeError("process_dev: integrate takes n, walk, rate_sign, dt, m and spread, not %s" % sorted(integrate))
        shift = walk_shifts(self.scales[2], dt, self.scales[3], n, rate_sign) if walk and n > 1 else None
        return n, shift, (None if m is None else int(m)), spread

    def _integrator(self, part, plane, n, m=None, spread=0):
        """The processor's Integrator of one (part, plane), on the engine's context."""
        from .integrate import Integrator
        if (part, plane) not in self._integ:
            self._integ[(part, plane)] = Integrator(engine=self.eng, n=n, m=m, spread=spread)
        return self._integ[(part, plane)]

    def _integrate(self, echo, out, opts, detector, with_flagV):
        """PC and MTD only, the sum and diff planes integrated per part, the flags from the integrated
        sum (and, with m, counted over the CPIs)."""
        import torch
        n, shift, m, spread = opts
        key = (n, m, spread)
        if key != self._integ_opts:
            self._integ = {}
            self._integ_opts = key
        ps, R_out = self.spec.cfar_segments[0][1], self.spec.R_out
        parts = (("short", (0, ps)), ("long", (ps, R_out)))
        out["sum_cpi"], out["diff_cpi"] = torch.empty_like(out["sum"]), torch.empty_like(out["diff"])
        self.eng.run_dev(echo, rdm=out["sum_cpi"], diff=out["diff_cpi"], cfar=None)
        # the parts are separate column windows: both start near zero range, no walk may cross column ps
        for plane in ("sum", "diff"):
            for part, cols in parts:
                self._integrator(part, plane, n).sum_dev(out[plane + "_cpi"], shift=shift, cols=cols, out=out[plane])
        if detector is None:
            self.eng.cfar_dev(out["sum"], out["flag"], flagV=out["flagV"] if with_flagV else None, cfar=self.cfar)
        else:
            from .oscfar import OsCfar
            if self._os is None:
                self._os = OsCfar(engine=self.eng)
            self._os.detect_dev(out["sum"], detector[0], detector[1], detector[2], flag=out["flag"], flagV=out["flagV"])
        if m is not None:
            for fk in ("flag", "flagV") if with_flagV or detector is not None else ("flag",):
                out[fk + "_cpi"] = out[fk]
                out[fk] = torch.empty_like(out[fk])
                for part, cols in parts:
                    self._integrator(part, fk, n, m, spread).count_dev(out[fk + "_cpi"], shift=shift, cols=cols,
                                                                         out=out[fk])
        return out

    def _detector_options(self, detector):
        """detector=dict(...) as (cfar, k, union): the preset's CFAR with T replaced when given."""
        import dataclasses
        detector = dict(detector)
        if "k" not in detector:
            raise TypeError("process_dev: detector needs k=(kV, kR)")
        k = tuple(int(x) for x in detector.pop("k"))
        union = tuple(bool(x) for x in detector.pop("union", (False, False)))
        T = detector.pop("T", None)
        if detector:
            raise TypeError("process_dev: detector takes k, union and T, not %s" % sorted(detector))
        cfar = self.cfar if T is None else dataclasses.replace(self.cfar, TV=float(T[0]), TR=float(T[1]))
        return cfar, k, union

    def process_dev(self, echo, beamPosNum, with_flagV=True, max_hits=4096, condense=None, width=None, track=None,
                    detector=None, integrate=None):
        """echo: complex64 [batch][2][P][R] (left, right) on the device.  Returns a dict of
        device outputs: the planes (sum, diff, flag, flagV) and, per part ('short', 'long') and
        flag kind ('flag', 'flagV'), (est, cells, count) as Measure.measure_dev gives them.

        condense = dict(gap=(gv, gr), wrap_v=False): the flags of each part and kind are first
        condensed into plots (Condense.condense_dev over the same column windows, amplitudes from
        the sum plane) and the measurement runs on the peak planes, one estimate per plot:
        out[(part, kind)] is the measurement of the peaks, out[(part, kind, 'plots')] =
        (plots, count) of the condensation (at most max_hits records per CPI), out['peak'] /
        out['peakV'] the peak planes.  wrap_v defaults to False: this layout has no fftshift, and
        its seam lies in the zeroed zero-velocity band.

        width = dict(amp_constr=-6.0, interp=4): every (part, kind) that is measured also gets
        out[(part, kind, 'width')] = (span, count) of Width.width_dev over the same column window
        of the sum plane (shift = 1: these planes carry no fftshift), on the columns of the flag
        plane that was measured (the peak plane when condensing), and out[(part, kind,
        'widthDots')], float64 [batch][max_hits]: the width of each measured hit's column, gathered
        through the measurement's cells, NaN past the count.

        track = dict(gate=(gate_r, gate_v), alpha=(ar, av, ae), confirm=(M, N), drop=(dt, dc),
        max_tracks=256, dt=P/prf, rate_sign=1.0): every (part, kind) that is measured also gets
        out[(part, kind, 'tracks')] = (assign, snap_f, snap_i, tcount) of Tracker.update_dev over
        that key's (est, count).  The processor owns one Tracker with a slot per (part, kind)
        (TRACK_SLOTS); its state persists from call to call, so the batches of successive calls are
        consecutive in time, and reset_tracks() clears it.  A call whose options differ from the
        previous call's starts a new Tracker.  Without condense every hit of a target starts its
        own track (a target lights several cells): track the plots, not the hits.  track=None
        leaves every other output as it is.

        detector = dict(k=(kV, kR), union=(False, False), T=(TV, TR)): the chain runs pulse
        compression and the MTD only, and flag / flagV come from one ordered-statistic CFAR call
        (OsCfar.detect_dev) over the whole sum plane with the preset's window, M0 and segments (T
        defaults to the preset's).  The measurement, condense, width and track run on those flags
        unchanged; flagV is always computed.  detector=None leaves the chain's own CFAR.

        integrate = dict(n=4, walk=True, rate_sign=1.0, dt=P/prf, m=None, spread=0): post-detection
        integration over the last n CPIs (rsp.integrate).  The chain runs pulse
        compression and the MTD only; out['sum_cpi'] / out['diff_cpi'] keep the per-CPI planes and
        out['sum'] / out['diff'] are their sums over the last n CPIs, the short and the long part as
        separate column windows, each past plane shifted row by row by its Doppler row's range walk
        (walk_shifts of vScale, dt and deltaR; walk=False: no shift).  The flags come from
        Engine.cfar_dev on the integrated sum with the preset's CFAR, or from `detector` when that is
        given as well; with m set they then pass the binary integration (at least m of the last n
        CPIs, within `spread` columns of the walked-back cell), out['flag_cpi'] / out['flagV_cpi']
        keeping what went in.  Condense, measure, width and track run unchanged on the results.  The
        processor holds one Integrator per (part, plane): the batches of successive calls are
        consecutive in time, reset_integration() clears the rings, and a call whose n, m or spread
        differ from the previous call's starts anew.  integrate=None leaves every output as it is."""
        import torch
        if integrate is not None:
            integrate = self._integrate_options(integrate)
        if detector is not None:
            detector = self._detector_options(detector)
        if track is not None:
            track = self._track_options(track)
        if width is not None:
            width = dict(width)
            wopt = (width.pop("amp_constr", -6.0), width.pop("interp", 4))
            if width:
                raise TypeError("process_dev: width takes amp_constr and interp, not %s" % sorted(width))
            width = wopt
        B = echo.shape[0]
        shp = (B, self.spec.V, self.spec.R_out)
        dev = self.device
        out = {k: torch.empty(shp, dtype=t, device=dev) for k, t in
               (("sum", torch.float32), ("diff", torch.float32), ("flag", torch.uint8), ("flagV", torch.uint8))}
        if integrate is not None:
            self._integrate(echo, out, integrate, detector, with_flagV)
        elif detector is None:
            self.eng.run_dev(echo, rdm=out["sum"], diff=out["diff"], flag=out["flag"],
                             flagV=out["flagV"] if with_flagV else None, cfar=self.cfar)
        else:
            from .oscfar import OsCfar
            if self._os is None:
                self._os = OsCfar(engine=self.eng)
            self.eng.run_dev(echo, rdm=out["sum"], diff=out["diff"], cfar=None)
            self._os.detect_dev(out["sum"], detector[0], detector[1], detector[2], flag=out["flag"], flagV=out["flagV"])
        rS, rL, vS, dR, dV = self.scales
        o = self.o
        k_value = float(self.kValues[self.freInd, int(beamPosNum)])
        p = self.meas.params(o["extraDots"], dR, o["rInterpTimes"], dV, o["vInterpTimes"], k_value, beamPosNum,
                             o["beamAngleStep"], o["eleAngleComp"], o["eleAngleSysErr"], self.spec.radar["M0"])
        ps = self.spec.cfar_segments[0][1]
        if condense is not None:
            out = self._measure_plots(out, p, ps, with_flagV, max_hits, dict(condense), width)
            return out if track is None else self._tracks(out, track, with_flagV)
        for fk in ("flag", "flagV") if with_flagV else ("flag",):
            for part, cols, rs in (("short", (0, ps), rS), ("long", (ps, self.spec.R_out), rL)):
                out[(part, fk)] = self.meas.measure_dev(out["sum"], out["diff"], out[fk], p, rs, vS,
                                                        max_hits=max_hits, cols=cols)
                if width is not None:
                    self._widths(out, part, fk, out[fk], cols, width)
        return out if track is None else self._tracks(out, track, with_flagV)

    def _widths(self, out, part, fk, flag, cols, width):
        """The widths of the columns of `flag` inside the window, and each measured hit's."""
        import torch
        from .width import Width, width_dots
        if self._width is None:
            self._width = Width(self.device.index or 0)
        amp_constr, interp = width
        span, count = self._width.width_dev(out["sum"], flag, amp_constr, interp, True, cols=cols)
        out[(part, fk, "width")] = (span, count)
        _, cells, n = out[(part, fk)]
        max_hits = cells.shape[1]
        wd = width_dots(span, interp)                                   # [batch][R]
        col = cells[:, :, 1].to(torch.int64).clamp_(0, span.shape[1] - 1)   # entries past the count are not written
        got = torch.gather(wd, 1, col) if max_hits else wd[:, :0]
        live = torch.arange(max_hits, device=wd.device)[None, :] < n[:, :1].to(torch.int64)
        out[(part, fk, "widthDots")] = torch.where(live, got, torch.full_like(got, float("nan")))

    def _measure_plots(self, out, p, ps, with_flagV, max_hits, cond, width=None):
        import torch
        from .condense import Condense
        if self._cond is None:
            self._cond = Condense(self.device.index or 0)
        gap, wrap_v = cond.pop("gap", (1, 1)), cond.pop("wrap_v", False)
        if cond:
            raise TypeError("process_dev: condense takes gap and wrap_v, not %s" % sorted(cond))
        rS, rL, vS = self.scales[:3]
        for fk, pk in (("flag", "peak"), ("flagV", "peakV")) if with_flagV else (("flag", "peak"),):
            out[pk] = torch.empty_like(out[fk])
            for part, cols, rs in (("short", (0, ps), rS), ("long", (ps, self.spec.R_out), rL)):
                _, plots, count = self._cond.condense_dev(out["sum"], out[fk], gap=gap, wrap_v=wrap_v,
                                                          max_plots=max_hits, cols=cols, peak=out[pk])
                out[(part, fk, "plots")] = (plots, count)
                out[(part, fk)] = self.meas.measure_dev(out["sum"], out["diff"], out[pk], p, rs, vS,
                                                        max_hits=max_hits, cols=cols)
                if width is not None:
                    self._widths(out, part, fk, out[pk], cols, width)
        return out

    def process_records_dev(self, d_stream, nbytes, nframes, with_flagV=True, max_hits=4096, condense=None,
                            width=None, track=None, detector=None, integrate=None):
        """:307-310 + process_dev from the record bytes: d_stream holds nframes * P consecutive
        legacy records (uint8 on the device, 4-byte aligned; the layout assumed for this waveform,
        see the module docstring), decoded into [nframes][2][P][R] without leaving HBM.  As the main
        does, each frame's beamPosNum and freInd are those of its last PRT; a frame whose freInd is
        not this processor's raises ValueError (its scales and k value would be another
        frequency's), and so does a stream that ends inside a frame.  The angle codes get
        angleCode = rem(angleCode + northAngle + angleE1, 360) (:310) on the host.
        process_dev measures a batch at one beam position, so the frames are processed in runs of
        consecutive frames that share beamPosNum.  Returns a list with one dict per run:
        process_dev's outputs for the run's frames plus 'frames' (first, end), 'beamPosNum',
        'frameInd' (int64 [n]) and 'angleCode' (float64 [n][P], host).  condense, width, track, detector,
        integrate: as process_dev's; the runs at different beamPosNum feed the same track slots, because the frames
        are consecutive in time and eleAngleEst is absolute."""
        from . import _capi as capi
        from .ingest import LegacyIngest
        if self._ingest is None:
            self._ingest = LegacyIngest(self.device.index or 0)
        P, R, F = self.spec.P, self.spec.R, int(nframes)
        echo, angle, head, status = self._ingest.decode_dev(d_stream, nbytes, P, R, F)
        decoded = int(status[F * P].item())
        if decoded < F * P:
            raise ValueError("process_records_dev: the stream ends inside PRT %d of frame %d" % (decoded % P + 1, decoded // P))
        last = head[:, P - 1].cpu().numpy()
        fre = last[:, capi.RSP_LEGACY_FRE_IND]
        if np.any(fre != self.freInd):
            f = int(np.flatnonzero(fre != self.freInd)[0])
            raise ValueError("process_records_dev: frame %d has freInd %d, this processor's is %d" % (f, int(fre[f]), self.freInd))
        bpn = last[:, capi.RSP_LEGACY_BEAM_POS_NUM]
        frame_ind = last[:, capi.RSP_LEGACY_FRAME_IND].astype(np.int64) & 0xffffffff
        code = np.fmod(angle.cpu().numpy() + self.o["northAngle"] + self.o["angleE1"], 360.0)
        runs, a = [], 0
        for b in range(1, F + 1):
            if b == F or bpn[b] != bpn[a]:
                out = self.process_dev(echo[a:b], int(bpn[a]), with_flagV=with_flagV, max_hits=max_hits,
                                       condense=condense, width=width, track=track, detector=detector,
                                       integrate=integrate)
                out.update(frames=(a, b), beamPosNum=int(bpn[a]), frameInd=frame_ind[a:b], angleCode=code[a:b])
                runs.append(out)
                a = b
        return runs
