"""Simulated targets injected into an echo at a set signal-to-clutter ratio on the GPU: the
target-injection step of MatlabProcess_xuzerui/main.m:183-194, which makes the truth R, V that
main_cfar.m's evaluation functions (rsp.score) score against, with the reference's names:

  * fun_SCR(prtNum, Echo_simu, echoData_Frame_0, SCR) -> Echo_simu_STC           fun_SCR.m: per
    segment (1:82, 83:324, 325:1031 with SCR + [10 0 0] dB) and per pulse, the target scaled by
    sqrt(P_echo * 10^(SCR/10) / P_s), P_s from the target's row 1, P_echo from the echo's row.
  * fun_add_clutter(Echo_simu_STC, echoData_Frame_0) -> echo                      fun_add_clutter.m:
    Echo_simu + echo(:, 1:point_prt).
  * Injector.scr_dev(simu, clutter, SCR, segments, ...): both in one pass over a device batch
    (rsp_scr_dev), any segments, a SCR per CPI.
  * Injector.inject_dev(clutter, plan, SCR): the point-target form (rsp_inject_dev): the target
    is formed in the kernel from a Plan (target_plan), 8 B read + 8 B written per sample.
  * target_plan(spec, Range, Velocity): one truth per CPI -> delays per segment, Doppler phase
    step and the waveforms on the device; Plan.truth_cells(spec, seg) are the cells for
    Scorer.score_dev.

The two quirks (include/rsp.h has the full text): `.^2` of complex I/Q data is the complex
square, so fun_SCR as written computes a complex gain -- power=AS_WRITTEN, the default of the
fun_SCR mirror; power=ABS2 uses |x|^2 and achieves the set SCR, the default elsewhere.  The body
of fun_SimulateTarget is not in the reference; the target is the point-target model of
rsp.synth (the segment's waveform at a delay column, times exp(j dphi m) at pulse m).

No CPU fallback: the injection runs only in librsp.so.
"""
import ctypes as C
import dataclasses
import math

import numpy as np

from . import _capi as capi

ABS2, AS_WRITTEN = capi.RSP_SCR_ABS2, capi.RSP_SCR_AS_WRITTEN
LEGACY_SEGMENTS = ((0, 82), (82, 242), (324, 707))   # (start, length), 0-based: 1:82, 83:324, 325:1031
LEGACY_SEG_DB = (10.0, 0.0, 0.0)                      # SCRs = [SCR+10 SCR SCR] (fun_SCR.m:23)


def scr_params(segments, seg_db=None, power=ABS2, add_clutter=True, clutter_ld=0, clutter_batch=0):
    """rsp_scr_params from segments = [(start, length), ...] (0-based columns)."""
    segments = list(segments)
    if len(segments) > capi.RSP_MAX_SEG:
        raise ValueError("at most %d segments (got %d)" % (capi.RSP_MAX_SEG, len(segments)))
    seg_db = [0.0] * len(segments) if seg_db is None else list(seg_db)
    if len(seg_db) != len(segments):
        raise ValueError("%d seg_db values for %d segments" % (len(seg_db), len(segments)))
    p = capi.rsp_scr_params()
    p.nseg, p.power, p.add_clutter = len(segments), int(power), int(bool(add_clutter))
    for i, (a, n) in enumerate(segments):
        p.seg_start[i], p.seg_len[i], p.seg_db[i] = int(a), int(n), float(seg_db[i])
    p.clutter_ld, p.clutter_batch = int(clutter_ld), int(clutter_batch)
    return p


def _mround(x):
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def waveforms(spec):
    """The point target's waveform per pulse-compression segment, as rsp.synth has it: the
    matched filter's replica normalised to peak 1, four ones for the FIR segment."""
    out = []
    for s in spec.segments:
        if s.kind == capi.RSP_SEG_FIR:
            out.append(np.ones(4, np.complex64))
        else:
            w = np.asarray(s.coef, np.complex128)
            out.append((w / np.max(np.abs(w))).astype(np.complex64))
    return out


@dataclasses.dataclass
class Plan:
    """One point target per CPI (target_plan).  Host copies next to the device tensors."""
    segments: list            # [(start, length)] of the echo row: the PC segments' input columns
    seg_db: list
    wf_host: list             # complex64 waveform per segment
    wf_off: np.ndarray        # int64 [nseg+1]
    delay: np.ndarray         # int32 [batch][RSP_MAX_SEG], -1 = no target in that segment
    dphi: np.ndarray          # float64 [batch]
    Range: np.ndarray
    Velocity: np.ndarray
    wf_dev: object = None
    delay_dev: object = None
    dphi_dev: object = None

    @property
    def batch(self):
        return self.delay.shape[0]

    def to(self, device):
        """Upload the waveforms, delays and phase steps (once; inject_dev does it on first use)."""
        import torch
        dev = torch.device(device)
        if self.wf_dev is None or self.wf_dev.device != dev:
            wf = np.concatenate(self.wf_host) if self.wf_host else np.zeros(0, np.complex64)
            self.wf_dev = torch.from_numpy(np.ascontiguousarray(wf, np.complex64)).to(dev)
            self.delay_dev = torch.from_numpy(self.delay).to(dev)
            self.dphi_dev = torch.from_numpy(self.dphi).to(dev)
        return self

    def truth_cells(self, spec, seg, gate=None):
        """int32 [batch][3] = {v_idx, r_idx, valid} for Scorer.score_dev, the target of segment
        `seg`: Doppler row round(2 v / lambda * P * prt) + P // 2 (the fftshift-ed RDM), the RDM
        column that the delay column maps to (out_start - in_start further), valid = the gate of
        score.truth_index (and a target in that segment at all)."""
        from . import score
        if spec.concat:
            raise ValueError("truth_cells: the range concatenation moves the columns (spec.concat)")
        if not spec.fftshift:
            raise ValueError("truth_cells: the Doppler row assumes an fftshift-ed RDM (spec.fftshift == 0)")
        g = score.GATE if gate is None else gate
        rp = spec.radar
        s = spec.segments[seg]
        out = np.zeros((self.batch, 3), np.int32)
        for b in range(self.batch):
            v, r, d = float(self.Velocity[b]), float(self.Range[b]), int(self.delay[b, seg])
            out[b, 0] = int(round(2 * v / rp["wavelength"] * spec.P * rp["prt"])) + spec.P // 2
            out[b, 1] = s.out_start + d if d >= 0 else 0
            out[b, 2] = int(d >= 0 and g[0] < abs(v) < g[1] and g[2] < r < g[3])
        return out


def target_plan(spec, Range, Velocity, r0=None, seg_db=None, device=None):  # noqa: N803
    """A Plan from vectors of one truth (Range [m], Velocity [m/s]) per CPI.  In segment s the
    target's waveform starts round((Range - r0[s]) / deltaR) columns after the segment's first
    input column (r0 defaults to 0 for every segment); a delay outside the segment means no
    target there (-1); a waveform that runs past the segment's end is truncated by the kernel.
    dphi = 2 pi (2 v / lambda) PRT.  device: upload now (else on first use)."""
    rp = spec.radar
    Rt = np.atleast_1d(np.asarray(Range, np.float64))
    Vt = np.atleast_1d(np.asarray(Velocity, np.float64))
    if Rt.shape != Vt.shape or Rt.ndim != 1:
        raise ValueError("target_plan: Range %s and Velocity %s must be vectors of one length" % (Rt.shape, Vt.shape))
    nseg = len(spec.segments)
    r0 = [0.0] * nseg if r0 is None else [float(x) for x in r0]
    if len(r0) != nseg:
        raise ValueError("target_plan: %d r0 values for %d segments" % (len(r0), nseg))
    deltaR = rp.get("deltaR", 2.99792458e8 / (2 * rp.get("fs", 25e6)))
    delay = np.full((Rt.size, capi.RSP_MAX_SEG), -1, np.int32)
    for b in range(Rt.size):
        for s, g in enumerate(spec.segments):
            d = _mround((Rt[b] - r0[s]) / deltaR)
            if 0 <= d < g.in_len:
                delay[b, s] = d
    wf = waveforms(spec)
    off = np.zeros(nseg + 1, np.int64)
    off[1:] = np.cumsum([len(w) for w in wf])
    plan = Plan(segments=[(g.in_start, g.in_len) for g in spec.segments],
                seg_db=[0.0] * nseg if seg_db is None else [float(x) for x in seg_db],
                wf_host=wf, wf_off=off, delay=delay,
                dphi=2.0 * np.pi * (2.0 * Vt / rp["wavelength"]) * rp["prt"], Range=Rt, Velocity=Vt)
    if device is not None:
        plan.to(device)
    return plan


class Injector:
    """rsp_scr_dev / rsp_inject_dev on a context of its own (the CFAR-only kind) or on an Engine's."""

    def __init__(self, device=0, engine=None):
        import torch
        self.lib = capi.load_library()
        self._engine = engine
        if engine is not None:
            self.ctx = engine.ctx
            device = engine.device
        else:
            ctx = C.c_void_p()
            capi.check(self.lib.rsp_create(C.byref(ctx), int(device), None), None)
            self.ctx = ctx
        self.device = torch.device("cuda", device)

    def close(self):
        if getattr(self, "ctx", None) and self._engine is None:
            self.lib.rsp_destroy(self.ctx)
        self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _echo(self, x):
        import torch
        if isinstance(x, torch.Tensor):
            return x.to(self.device, torch.complex64)
        a = np.ascontiguousarray(x, dtype=np.complex64)
        return torch.from_numpy(a if a.flags.writeable else a.copy()).to(self.device)

    def _scr(self, SCR, batch):  # noqa: N803
        import torch
        if isinstance(SCR, torch.Tensor):
            s = SCR.to(self.device, torch.float64).reshape(-1)
        else:
            s = torch.as_tensor(np.asarray(SCR, np.float64).reshape(-1), device=self.device)
        if s.numel() == 1 and batch != 1:
            s = s.expand(batch)
        if s.numel() != batch:
            raise ValueError("%d SCR values for %d CPIs" % (s.numel(), batch))
        return s.contiguous()

    def _clutter(self, clutter, P, R):
        """-> (tensor, batch K, row pitch): [K][P][ld] with unit column stride (a column window
        of a wider echo is taken in place, fun_add_clutter's echo(:, 1:point_prt))."""
        c = self._echo(clutter)
        if c.dim() == 2:
            c = c[None]
        if c.dim() != 3 or c.shape[1] != P or c.shape[2] != R:
            raise ValueError("clutter is %s, expected [K][%d][%d]" % (tuple(c.shape), P, R))
        ld = c.stride(1)
        if c.stride(2) != 1 or ld < R or (c.shape[0] > 1 and c.stride(0) != P * ld):
            c = c.contiguous()
            ld = R
        return c, c.shape[0], ld

    def _out(self, out, shape):
        import torch
        if out is None:
            return torch.empty(shape, dtype=torch.complex64, device=self.device)
        if tuple(out.shape) != tuple(shape) or out.dtype != torch.complex64 or not out.is_contiguous() or \
                out.device != self.device:
            raise ValueError("out must be a contiguous complex64 tensor of shape %s on %s" % (tuple(shape), self.device))
        return out

    def _stream(self, stream):
        import torch
        return C.c_void_p(stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream)

    def scr_dev(self, simu, clutter, SCR, segments, seg_db=None, power=ABS2, add_clutter=True, out=None,  # noqa: N803
                stream=None):
        """simu complex64 [batch][P][R] (or [P][R]); clutter [K][P][>=R], K <= batch (CPI b uses
        clutter b % K); SCR in dB, a scalar or one per CPI; segments [(start, length)].  Returns
        out = sqrt(g) .* simu + clutter (add_clutter=False: the scaled target alone); out may be
        simu, or clutter when K == batch and its rows are R wide.  Asynchronous on `stream`."""
        x = self._echo(simu)
        if x.dim() == 2:
            x = x[None]
        if x.dim() != 3:
            raise ValueError("simu must be [batch][P][R] (got %s)" % (tuple(x.shape),))
        x = x.contiguous()
        B, P, R = x.shape
        c, K, ld = self._clutter(clutter, P, R)
        o = self._out(out, x.shape)
        scr = self._scr(SCR, B)
        p = scr_params(segments, seg_db, power, add_clutter, clutter_ld=ld, clutter_batch=K)
        capi.check(self.lib.rsp_scr_dev(self.ctx, x.data_ptr(), c.data_ptr(), o.data_ptr(), P, R, B, scr.data_ptr(),
                                        C.byref(p), self._stream(stream)), self.ctx)
        self._keep = (x, c, scr)   # alive until the caller synchronises
        return o

    def inject_dev(self, clutter, plan, SCR, out=None, power=ABS2, add_clutter=True, stream=None):  # noqa: N803
        """The plan's point targets at SCR dB (a scalar or one per CPI) over clutter [K][P][>=R],
        K <= plan.batch.  Returns out [plan.batch][P][R]; out may be clutter when K == batch and
        its rows are R wide.  Asynchronous on `stream`."""
        c = self._echo(clutter)
        if c.dim() == 2:
            c = c[None]
        P, R = c.shape[-2], c.shape[-1]
        c, K, ld = self._clutter(c, P, R)
        B = plan.batch
        plan.to(self.device)
        o = self._out(out, (B, P, R))
        scr = self._scr(SCR, B)
        p = scr_params(plan.segments, plan.seg_db, power, add_clutter, clutter_ld=ld, clutter_batch=K)
        off = (C.c_int64 * len(plan.wf_off))(*[int(v) for v in plan.wf_off])
        capi.check(self.lib.rsp_inject_dev(self.ctx, c.data_ptr(), o.data_ptr(), P, R, B, plan.wf_dev.data_ptr(), off,
                                           plan.delay_dev.data_ptr(), plan.dphi_dev.data_ptr(), scr.data_ptr(),
                                           C.byref(p), self._stream(stream)), self.ctx)
        self._keep = (c, scr, plan)
        return o

    # ---- the reference's own functions -----------------------------------------------------
    def fun_SCR(self, prtNum, Echo_simu, echoData_Frame_0, SCR, segments=LEGACY_SEGMENTS,  # noqa: N802,N803
                seg_db=LEGACY_SEG_DB, power=AS_WRITTEN):
        """fun_SCR.m on prtNum x point_prt matrices (rows = pulses): Echo_simu_STC as a device
        tensor.  As written: complex squares and the principal root (power=ABS2 for |x|^2).
        The echo may be wider than Echo_simu; its first columns are used."""
        x = self._echo(Echo_simu)
        if x.dim() != 2 or x.shape[0] != int(prtNum):
            raise ValueError("fun_SCR: Echo_simu is %s, expected %d rows" % (tuple(x.shape), int(prtNum)))
        e = self._echo(echoData_Frame_0)
        if e.dim() != 2 or e.shape[0] < x.shape[0] or e.shape[1] < x.shape[1]:
            raise ValueError("fun_SCR: the echo %s is smaller than Echo_simu %s (MATLAB: index error)"
                             % (tuple(e.shape), tuple(x.shape)))
        return self.scr_dev(x, e[:x.shape[0], :x.shape[1]], SCR, segments, seg_db, power, add_clutter=False)[0]

    def fun_add_clutter(self, Echo_simu_STC, echoData_Frame_0):  # noqa: N802,N803
        """fun_add_clutter.m: Echo_simu(i, :) + echo(i, 1:point_prt) for every row of Echo_simu."""
        x = self._echo(Echo_simu_STC)
        e = self._echo(echoData_Frame_0)
        if x.dim() != 2 or e.dim() != 2 or e.shape[0] < x.shape[0] or e.shape[1] < x.shape[1]:
            raise ValueError("fun_add_clutter: the echo %s is smaller than Echo_simu %s (MATLAB: index error)"
                             % (tuple(e.shape), tuple(x.shape)))
        return self.scr_dev(x, e[:x.shape[0], :x.shape[1]], 0.0, segments=())[0]   # no segment: gain 1 everywhere
