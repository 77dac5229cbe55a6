"""Doppler line width per range column on the GPU: how wide a Doppler spectrum
stands above a level set in dB below its own peak, optionally on a spline-refined grid, through
rsp_spec_width_dev (csrc/rsp_width.hip).  With the reference's name and argument meaning:

  * ampConstrWidthEst(specData, ampConstr, interpFlag, interpTimes) -> widthDots
    MatlabProcess_xuzerui/CFAR_WangCai/ampConstrWidthEst.m:1-45 (the figures and the
    commented-out walk from the peak are not part of it): y = abs(fftshift(specData)), the
    not-a-knot spline of y sampled every 1/interpTimes, the span of the samples within ampConstr
    dB of the maximum.
  * Width.width_dev(amp, flag, amp_constr, interp, shift, cols=None) -> (span, count): the batched
    device form over [batch][V][R] planes (optionally a column window of wider planes), one
    {first, last} pair per column that carries a hit, {-1, -1} elsewhere.
  * width_dots(span, interp): (last - first) / interp, 0 where the span is {-1, -1}.

No CPU fallback: the widths are computed only in librsp.so.
"""
import ctypes as C

import numpy as np

from . import _capi as capi


def width_dots(span, interp):
    """widthDots float64 [...] of spans int32 [..., 2] (a tensor or an array): (last - first) /
    interp; an uncomputed or all-zero column's {-1, -1} gives 0, as the reference's empty set."""
    if isinstance(span, np.ndarray):
        return (span[..., 1].astype(np.float64) - span[..., 0].astype(np.float64)) / float(interp)
    import torch
    return (span[..., 1].to(torch.float64) - span[..., 0].to(torch.float64)) / float(interp)


class Width:
    """Owns an rsp context (the CFAR-only kind) for rsp_spec_width_dev."""

    def __init__(self, device=0):
        import torch
        self.lib = capi.load_library()
        self.device = torch.device("cuda", device)
        ctx = C.c_void_p()
        capi.check(self.lib.rsp_create(C.byref(ctx), int(device), None), None)
        self.ctx = ctx

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.rsp_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dev(self, x, dtype):
        import torch
        if isinstance(x, torch.Tensor):
            return x.to(self.device, dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(x), device=self.device).to(dtype).contiguous()

    def width_dev(self, amp, flag, amp_constr, interp, shift, cols=None, stream=None):
        """amp float32 [batch][V][Rp] (magnitudes), flag uint8 [batch][V][Rp] or None (device
        tensors, or arrays copied to the device; nonzero = hit, None = every column).  cols =
        (lo, hi) takes the column window lo..hi-1 of every plane in place, as
        Measure.measure_dev does.  shift: fftshift each column first (the DMX planes carry no
        shift; the v2 / legacy RDM is already centred).  Returns (span int32 [batch][R][2] =
        {first, last} on the 1/interp grid, {-1, -1} for a column without a hit or without a
        positive maximum; count int32 [batch], the columns computed) on the device, asynchronous
        on `stream` (default: torch's current stream)."""
        import torch
        a = self._dev(amp, torch.float32)
        f = None if flag is None else self._dev(flag, torch.uint8)
        if a.dim() == 2:
            a = a[None]
            f = None if f is None else f[None]
        B, V, Rp = a.shape
        if f is not None and f.shape != a.shape:
            raise ValueError("width_dev: amp %s and flag %s differ in shape" % (tuple(a.shape), tuple(f.shape)))
        lo, hi = (0, Rp) if cols is None else (int(cols[0]), int(cols[1]))
        if not 0 <= lo < hi <= Rp:
            raise ValueError("width_dev: column window %r outside 0..%d" % ((lo, hi), Rp))
        R = hi - lo
        span = torch.empty((B, R, 2), dtype=torch.int32, device=self.device)
        count = torch.empty((B,), dtype=torch.int32, device=self.device)
        p = capi.rsp_width_params()
        p.amp_constr, p.interp, p.shift = float(amp_constr), int(interp), int(bool(shift))
        p.ld, p.cpi_stride = Rp, V * Rp
        st = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.rsp_spec_width_dev(
            self.ctx, a.data_ptr() + 4 * lo, None if f is None else f.data_ptr() + lo, V, R, B, C.byref(p),
            span.data_ptr(), count.data_ptr(), C.c_void_p(st)), self.ctx)
        self._keep = (a, f)    # alive until the caller synchronises
        return span, count

    def ampConstrWidthEst(self, specData, ampConstr, interpFlag, interpTimes):  # noqa: N802 (reference name)
        """ampConstrWidthEst.m for a 1-D spectrum, or the columns of a 2-D [V][n] one (complex or
        real; abs is taken on the host): widthDots as float64, a scalar or [n] (synchronises)."""
        x = np.asarray(specData)
        one = x.ndim == 1
        if x.ndim not in (1, 2):
            raise ValueError("ampConstrWidthEst: specData must be 1-D or 2-D [V][n]")
        a = np.abs(x).astype(np.float32).reshape(x.shape[0], -1)
        interp = int(interpTimes) if interpFlag else 1
        span, _ = self.width_dev(a, None, ampConstr, interp, True)
        w = width_dots(span[0].cpu().numpy(), interp)
        return float(w[0]) if one else w


def ampConstrWidthEst(specData, ampConstr, interpFlag, interpTimes, device=0):  # noqa: N802 (reference name)
    """ampConstrWidthEst.m on the GPU `device` (a Width of its own for the call)."""
    w = Width(device)
    try:
        return w.ampConstrWidthEst(specData, ampConstr, interpFlag, interpTimes)
    finally:
        w.close()
