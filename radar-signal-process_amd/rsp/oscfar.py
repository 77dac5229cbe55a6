"""Ordered-statistic CFAR on the GPU: a second detector beside the chain's
greatest-of / smallest-of cell-averaging one, through rsp_os_cfar_dev (csrc/rsp_oscfar.hip).

The stage is executeCFAR.m (CFAR_WangCai/executeCFAR.m:1-93, Function_CFAR1D_sub.m) with one
substitution: the noise estimate of a reference window is its k-th smallest cell, not its mean, and
the threshold is T times that cell (T is not divided by ref).  Row band, column segments, the
zero_v_div rows, the one-sided windows at the edges, the range test on r-1, r, r+1 of every Doppler
hit and the first-maximum re-localisation are the existing detector's.

  * OsCfar.detect_dev(rdm, cfar, k=(kV, kR), union=(False, False), flag=None, flagV=None,
    cols=None) -> (flag, flagV): the batched device form over [batch][V][Rp] planes (optionally a
    column window of wider planes, in place).  Per side (union False) k is 1..ref and the two
    sides' k-th smallest cells combine by cfar.methodV / methodR (0 greatest-of, 1 smallest-of);
    with union True k is 1..2*ref over both sides as one set.
  * OsCfar.plan(V, R, batch, cfar, k, union, flagV=True): the launches that call would make.
  * detector(os, k, union, T=None): a callable (rdm, flag, cfar) for rsp.score.sweep / scr_sweep.

No CPU fallback: the flags are computed only in librsp.so.
"""
import ctypes as C
import dataclasses

import numpy as np

from . import _capi as capi


def os_params(k, union=(False, False)):
    """rsp_os_params of k = (kV, kR) and union = (unionV, unionR); the geometry is left 0."""
    p = capi.rsp_os_params()
    p.kV, p.kR = int(k[0]), int(k[1])
    p.unionV, p.unionR = int(bool(union[0])), int(bool(union[1]))
    return p


class OsCfar:
    """Owns an rsp context (the CFAR-only kind) for rsp_os_cfar_dev, or borrows an Engine's."""

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

    def _dev(self, x, dtype):
        import torch
        if isinstance(x, torch.Tensor):
            return x.to(self.device, dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(x), device=self.device).to(dtype).contiguous()

    def detect_dev(self, rdm, cfar, k, union=(False, False), flag=None, flagV=None, cols=None, stream=None):
        """rdm float32 [batch][V][Rp] (magnitudes; a device tensor, or an array copied to the
        device), cfar a presets.Cfar whose ref / guard / T / method / M0 / rFlag / zero_v_div /
        segments keep their meaning (segments are relative to the window), k = (kV, kR) the
        1-based ranks, union = (unionV, unionR).  flag / flagV: uint8 tensors of rdm's shape to
        write into (default: new ones; columns outside the window keep their bytes, new tensors
        are zeroed there).  cols = (lo, hi) takes the column window lo..hi-1 of every plane in
        place, as Width.width_dev does.  Returns (flag, flagV) on the device, asynchronous on
        `stream` (default: torch's current stream)."""
        import torch
        a = self._dev(rdm, torch.float32)
        if a.dim() == 2:
            a = a[None]
        if a.dim() != 3:
            raise ValueError("detect_dev: rdm %s must be [batch][V][R]" % (tuple(a.shape),))
        B, V, Rp = a.shape
        lo, hi = (0, Rp) if cols is None else (int(cols[0]), int(cols[1]))
        if not 0 <= lo < hi <= Rp:
            raise ValueError("detect_dev: column window %r outside 0..%d" % ((lo, hi), Rp))
        outs = []
        for name, t in (("flag", flag), ("flagV", flagV)):
            if t is None:
                t = (torch.empty if cols is None else torch.zeros)((B, V, Rp), dtype=torch.uint8, device=self.device)
            elif (tuple(t.shape) != (B, V, Rp) or t.dtype != torch.uint8 or not t.is_contiguous()
                  or t.device != a.device):
                raise ValueError("detect_dev: %s must be a contiguous uint8 tensor of shape %s on %s"
                                 % (name, (B, V, Rp), a.device))
            outs.append(t)
        p = os_params(k, union)
        p.ld, p.cpi_stride = Rp, V * Rp
        cp = cfar.to_c()
        st = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.rsp_os_cfar_dev(
            self.ctx, a.data_ptr() + 4 * lo, V, hi - lo, B, C.byref(cp), C.byref(p), outs[0].data_ptr() + lo,
            outs[1].data_ptr() + lo, C.c_void_p(st)), self.ctx)
        self._keep = (a,)    # alive until the caller synchronises
        return outs[0], outs[1]

    def plan(self, V, R, batch, cfar, k, union=(False, False), flagV=True):
        """rsp_os_cfar_plan as a dict: the launches detect_dev would make for a V x R window."""
        p = os_params(k, union)
        cp = cfar.to_c()
        out = capi.rsp_os_plan_t()
        capi.check(self.lib.rsp_os_cfar_plan(self.ctx, int(V), int(R), int(batch), C.byref(cp), C.byref(p),
                                             int(bool(flagV)), C.byref(out)), self.ctx)
        return {f: getattr(out, f) for f, _ in out._fields_ if f != "reserved"}


def detector(os, k, union=(False, False), T=None):
    """A callable (rdm, flag, cfar) for rsp.score.sweep / scr_sweep's `detector`: OsCfar `os`
    with ranks k and forms union; T = (TV, TR), if given, replaces cfar's thresholds."""
    def run(rdm, flag, cfar):
        c = cfar if T is None else dataclasses.replace(cfar, TV=float(T[0]), TR=float(T[1]))
        os.detect_dev(rdm, c, k, union, flag=flag)
    return run
