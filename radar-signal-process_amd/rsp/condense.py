"""Plot condensation on the GPU: the CFAR hits of each CPI are labelled into
connected clusters ("plots") and each plot keeps its strongest cell, through rsp_condense_dev
(csrc/rsp_condense.hip).

  * Condense.condense_dev(amp, flag, gap, wrap_v, ...): the batched device form, [batch][V][R]
    in (optionally a column window of wider planes), (peak, plots, count) out.  peak is a flag
    plane with only the plots' peak cells set; Measure.measure_dev takes it in place of the CFAR
    flags, and its hit i is plot i.
  * Condense.plots(amp, flag, ...): one CPI, a numpy structured array of the plots.

Hits (v1, r1), (v2, r2) are adjacent when |v1 - v2| <= gap[0] (around the Doppler seam with
wrap_v) and |r1 - r2| <= gap[1]; a plot is a connected component; its peak is the hit with the
largest amplitude, the first in MATLAB's find() order among equals.  v_min / v_max are plain
minima and maxima of the row indices: a plot joined across the seam reports 0 and V-1.

No CPU fallback: the plots are computed only in librsp.so.
"""
import ctypes as C

import numpy as np

from . import _capi as capi

PLOT_DTYPE = np.dtype([(n, np.int32) for n in
                       ("peak_v", "peak_r", "n_cells", "v_min", "v_max", "r_min", "r_max", "reserved")])


class Condense:
    """Owns an rsp context (the CFAR-only kind) for rsp_condense_dev."""

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

    def condense_dev(self, amp, flag, gap=(1, 1), wrap_v=False, max_plots=None, cols=None, stream=None, peak=None):
        """amp float32 [batch][V][Rp], flag uint8 [batch][V][Rp] (device tensors, or arrays copied
        to the device; nonzero = hit).  cols = (lo, hi) condenses the column window lo..hi-1 of
        every plane in place, as Measure.measure_dev measures it; hits do not join across the
        window's edges.  peak: an existing uint8 plane of flag's shape to write the window of
        (default: a new one, zero outside the window).  Returns (peak uint8 [batch][V][Rp],
        plots int32 [batch][max_plots][8] = {peak_v, peak_r, n_cells, v_min, v_max, r_min, r_max,
        0} relative to the window, in the order Measure.measure_dev lists peak's hits, count int32
        [batch][2] = {n_plots, n_hits}) on the device.  Plots past max_plots are counted, not
        written; peak is complete all the same."""
        import torch
        a = self._dev(amp, torch.float32)
        f = self._dev(flag, torch.uint8)
        if a.dim() == 2:
            a, f = a[None], f[None]
        B, V, Rp = a.shape
        if f.shape != a.shape:
            raise ValueError("condense_dev: amp %s and flag %s differ in shape" % (tuple(a.shape), tuple(f.shape)))
        lo, hi = (0, Rp) if cols is None else (int(cols[0]), int(cols[1]))
        if not 0 <= lo < hi <= Rp:
            raise ValueError("condense_dev: column window %r outside 0..%d" % ((lo, hi), Rp))
        R = hi - lo
        if max_plots is None:
            max_plots = min(V * R, 1 << 16)
        if peak is None:
            peak = torch.empty((B, V, Rp), dtype=torch.uint8, device=self.device)
            if R != Rp:
                peak.zero_()
        elif (not isinstance(peak, torch.Tensor) or peak.dtype != torch.uint8 or tuple(peak.shape) != (B, V, Rp)
              or not peak.is_contiguous() or peak.device != f.device):
            raise ValueError("condense_dev: peak must be a contiguous uint8 device tensor of flag's shape")
        plots = torch.empty((B, max_plots, 8), dtype=torch.int32, device=self.device)
        count = torch.empty((B, 2), dtype=torch.int32, device=self.device)
        p = capi.rsp_condense_params()
        p.gap_v, p.gap_r, p.wrap_v = int(gap[0]), int(gap[1]), int(bool(wrap_v))
        p.ld, p.cpi_stride = Rp, V * Rp
        st = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.rsp_condense_dev(
            self.ctx, a.data_ptr() + 4 * lo, f.data_ptr() + lo, V, R, B, C.byref(p), peak.data_ptr() + lo,
            max_plots, plots.data_ptr(), count.data_ptr(), C.c_void_p(st)), self.ctx)
        self._keep = (a, f)    # alive until the caller synchronises
        return peak, plots, count

    def plots(self, amp, flag, gap=(1, 1), wrap_v=False, max_plots=4096, cols=None):
        """One V x R CPI: its plots as a numpy structured array (PLOT_DTYPE), in peak find()
        order; runs again with a larger max_plots when there are more (synchronises)."""
        _, pl, count = self.condense_dev(amp, flag, gap=gap, wrap_v=wrap_v, max_plots=max_plots, cols=cols)
        n = int(count[0, 0].item())
        if n > pl.shape[1]:
            _, pl, count = self.condense_dev(amp, flag, gap=gap, wrap_v=wrap_v, max_plots=n, cols=cols)
        return np.ascontiguousarray(pl[0, :n].cpu().numpy()).view(PLOT_DTYPE).reshape(n)
