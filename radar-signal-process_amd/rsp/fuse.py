"""The stacked beams' hits fused per cell, and the elevation from the beam amplitudes,
through rsp_beam_fuse_dev and rsp_beam_elev_dev (csrc/rsp_fuse.hip).

The v2 capture forms a stack of elevation beams and Engine.window_dev gives one RDM and one flag plane
per beam; a target is flagged in two or three neighbouring beams at the same (v, r).  BeamFuser merges
the flags per cell (a fused hit needs `min_beams` flagged beams), names the flagged beam with the
largest amplitude and keeps the largest amplitude of all beams as the plane that condensation and the
measurement run on; for each measured hit it then estimates the elevation from the peak beam and the
beam on either side (`law`), into the measurement's est[..., 2], which the tracker reads:

    fuser = BeamFuser(beam_el, min_beams=2)
    amp, flg = (t.flatten(1, 2).transpose(0, 1) for t in (rdm, flag))     # window_dev's outputs, no copy
    est, cells, count = fuser.plots_dev(amp, flg, (measure, params), r_scale, v_scale, condense=condense)

No CPU fallback: the planes are fused only in librsp.so.
"""
import ctypes as C

import numpy as np

from . import _capi as capi

LAWS = {"centre": 0, "center": 0, "centroid": 1, "logparab": 2}


class BeamFuser:
    """beam_el: the beam centres [deg], 2..32 of them, strictly monotonic.  min_beams: the flagged beams a
    cell needs to become a fused hit.  law: "centre" (the peak beam's centre), "centroid" (power centroid
    of the peak beam and its two neighbours) or "logparab" (the vertex of the parabola through the three
    log amplitudes: exact for Gaussian beams of one width), or 0 / 1 / 2.  Owns an rsp context (the
    CFAR-only kind), or borrows an Engine's."""

    def __init__(self, beam_el, min_beams=1, law="logparab", device=0, engine=None):
        import torch
        self.lib = capi.load_library()
        self.beam_el = np.asarray(beam_el, dtype=np.float64).reshape(-1)
        if not 2 <= self.beam_el.size <= capi.RSP_FUSE_MAX_BEAMS:
            raise ValueError("BeamFuser: %d beam centres, 2..%d are supported" % (self.beam_el.size, capi.RSP_FUSE_MAX_BEAMS))
        self.beams, self.min_beams = int(self.beam_el.size), int(min_beams)
        if isinstance(law, str):
            if law not in LAWS:
                raise ValueError("BeamFuser: law %r is none of %s" % (law, sorted(LAWS)))
            law = LAWS[law]
        self.law = int(law)
        # refuse malformed parameters before anything is allocated: a well-formed call without a
        # context gets as far as "null ctx"
        p = self._params(1, 1, self.beams)
        rc = self.lib.rsp_beam_fuse_dev(None, 1 << 40, 2 << 40, 1, 1, 1, C.byref(p), 3 << 40, 4 << 40, None, None, None)
        msg = (self.lib.rsp_last_error(None) or b"").decode()
        if "null ctx" not in msg:
            raise capi.RspError(rc, msg)
        self._engine = engine
        if engine is not None:
            self.ctx = engine.ctx
            device = engine.device
        else:
            ctx = C.c_void_p()
            capi.check(self.lib.rsp_create(C.byref(ctx), int(device), None), None)
            self.ctx = ctx
        self.device = torch.device("cuda", device)

    def _params(self, ld, bs, cs):
        p = capi.rsp_fuse_params()
        p.beams, p.min_beams, p.law, p.reserved = self.beams, self.min_beams, self.law, 0
        p.ld, p.beam_stride, p.cpi_stride = int(ld), int(bs), int(cs)
        for k, x in enumerate(self.beam_el):
            p.beam_el[k] = float(x)
        return p

    def close(self):
        if getattr(self, "ctx", None) and self._engine is None:
            self.lib.rsp_destroy(self.ctx)
        self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _planes(self, who, amp, flag):
        """The shape and the three strides of amp / flag [batch, beams, V, R], read off the tensors: nothing
        is copied, and a layout the three strides cannot express is refused."""
        import torch
        for name, t, dt in (("amp", amp, torch.float32), ("flag", flag, torch.uint8)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != self.device:
                raise ValueError("%s: %s must be a %s tensor on %s" % (who, name, dt, self.device))
        if amp.dim() != 4 or amp.shape[1] != self.beams or amp.shape != flag.shape:
            raise ValueError("%s: amp %s and flag %s must both be [batch, beams = %d, V, R]"
                             % (who, tuple(amp.shape), tuple(flag.shape), self.beams))
        B, _, V, R = (int(n) for n in amp.shape)
        if B < 1 or V < 1 or R < 1:
            raise ValueError("%s: empty planes %s" % (who, tuple(amp.shape)))

        def strides(t):
            sb, sk, sv, sr = (int(s) for s in t.stride())
            # a dimension of one element has no stride worth the name
            return (sb if B > 1 else 0, sk, sv if V > 1 else R, sr if R > 1 else 1)
        sa, sf = strides(amp), strides(flag)
        if sa != sf:
            raise ValueError("%s: amp (strides %s) and flag (strides %s) must share one layout" % (who, sa, sf))
        cs, bs, ld, sr = sa
        if sr != 1 or ld < R or bs < 1 or cs < 0:
            raise ValueError("%s: strides %s: the columns of a row must be adjacent, and the rows, beams and CPIs "
                             "each a fixed positive number of elements apart" % (who, tuple(amp.stride())))
        return B, V, R, ld, bs, cs

    def fuse_dev(self, amp, flag, out=None, stream=None):
        """amp float32, flag uint8 (nonzero = hit): device tensors [batch, beams, V, R] of one layout, the
        contiguous one or any view whose columns are adjacent and whose rows, beams and CPIs are fixed
        strides apart -- Engine.window_dev's [beams, F, win, V, R] outputs as
        rdm.flatten(1, 2).transpose(0, 1).  out: (fflag, fbeam, famp, fcnt) to write into, contiguous
        [batch, V, R] (uint8, uint8, float32, uint8).  Returns that tuple: the fused flags, the peak beam
        (255 off the hits), the largest amplitude of all beams and the number of flagged beams.
        Asynchronous on `stream` (default: torch's current stream)."""
        import torch
        B, V, R, ld, bs, cs = self._planes("fuse_dev", amp, flag)
        dts = (torch.uint8, torch.uint8, torch.float32, torch.uint8)
        if out is None:
            out = tuple(torch.empty((B, V, R), dtype=dt, device=self.device) for dt in dts)
        else:
            out = tuple(out)
            if len(out) != 4 or any(not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (B, V, R)
                                    or not t.is_contiguous() or t.device != self.device for t, dt in zip(out, dts)):
                raise ValueError("fuse_dev: out must be (fflag u8, fbeam u8, famp f32, fcnt u8), contiguous %s on %s"
                                 % ((B, V, R), self.device))
        p = self._params(ld, bs, cs)
        st = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.rsp_beam_fuse_dev(self.ctx, amp.data_ptr(), flag.data_ptr(), V, R, B, C.byref(p),
                                              out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                              C.c_void_p(st)), self.ctx)
        return out

    def elevation_dev(self, amp, flag, fbeam, cells, count, est=None, hb=None, stream=None):
        """The elevation of every listed hit.  amp, flag as fuse_dev's; fbeam its second output; cells int32
        [batch, max_hits, 2] and count int32 [batch, 2] as Measure.measure_dev returns them for famp with
        fflag or with a condensed peak plane.  est: the measurement's float64 [batch, max_hits, 3], whose
        [..., 2] is written (and est returned); without it a float64 [batch, max_hits] tensor is returned,
        NaN past each CPI's count.  hb: an int32 [batch, max_hits, 4] tensor to receive {peak beam,
        flagged beams, lower beam used, upper beam used} per hit."""
        import torch
        B, V, R, ld, bs, cs = self._planes("elevation_dev", amp, flag)

        def dense(name, t, dt, shape):
            if (not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()
                    or t.device != self.device):
                raise ValueError("elevation_dev: %s must be a contiguous %s tensor of shape %s on %s"
                                 % (name, dt, shape, self.device))
        if not isinstance(cells, torch.Tensor) or cells.dim() != 3:
            raise ValueError("elevation_dev: cells must be int32 [batch, max_hits, 2]")
        H = int(cells.shape[1])
        dense("fbeam", fbeam, torch.uint8, (B, V, R))
        dense("cells", cells, torch.int32, (B, H, 2))
        dense("count", count, torch.int32, (B, 2))
        if hb is not None:
            dense("hb", hb, torch.int32, (B, H, 4))
        if est is not None:
            dense("est", est, torch.float64, (B, H, 3))
            ret, ptr, stride = est, est.data_ptr() + 16, 3
        else:
            ret = torch.full((B, H), float("nan"), dtype=torch.float64, device=self.device)
            ptr, stride = ret.data_ptr(), 1
        p = self._params(ld, bs, cs)
        st = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.rsp_beam_elev_dev(self.ctx, amp.data_ptr(), flag.data_ptr(), fbeam.data_ptr(), V, R, B,
                                              C.byref(p), cells.data_ptr() if H else None, count.data_ptr(), H,
                                              ptr if H else None, stride, hb.data_ptr() if hb is not None and H else None,
                                              C.c_void_p(st)), self.ctx)
        return ret

    def plots_dev(self, amp, flag, measure, r_scale, v_scale, condense=None, max_hits=None):
        """The stacked planes of a batch of CPIs as plots for the tracker: fuse_dev; with `condense` (a
        Condense, or (Condense, dict of condense_dev's keywords)) the fused hits condensed to one peak cell
        per cluster on famp / fflag; `measure` = (Measure, rsp_measure_params from Measure.params) on famp,
        passed as both the sum and the difference plane, at the fused hits or the peaks; then
        elevation_dev into est[..., 2].  Returns (est, cells, count) as Measure.measure_dev does, ready for
        Tracker.  Everything runs on torch's current stream."""
        meas, params = measure
        fflag, fbeam, famp, _ = self.fuse_dev(amp, flag)
        hits = fflag
        if condense is not None:
            cond, kw = condense if isinstance(condense, (tuple, list)) else (condense, {})
            hits = cond.condense_dev(famp, fflag, **kw)[0]
        est, cells, count = meas.measure_dev(famp, famp, hits, params, r_scale, v_scale, max_hits=max_hits)
        self.elevation_dev(amp, flag, fbeam, cells, count, est=est)
        return est, cells, count
