"""Post-detection integration over the CPIs of a dwell, through rsp_integrate_dev and
rsp_binint_dev (csrc/rsp_integ.hip).

Every detector of the library decides on one CPI alone; a target below the threshold in each CPI of a
dwell is lost.  The Integrator sums the amplitude planes of the last n CPIs before the CFAR (video
integration, sum_dev) or counts the flag planes of the last n CPIs after it (binary M-of-N integration,
count_dev).  The RDM orders the cells by velocity, so Doppler row v has a known range walk per CPI
(walk_shifts): each past plane is shifted row by row before it is added, and the target piles up in one
cell.  The state stays on the device, `slots` independent rings:

    hist  float32 / uint8 [slots][n-1][V][R]   the last n-1 input planes of each slot (window columns)
    meta  int32           [slots][2]           {CPIs the slot has seen, 0}

The result of sum_dev is a sum, not a mean (include/rsp.h): the first n-1 CPIs of a slot come out at a
smaller scale, which the ratio tests behind it do not see.

No CPU fallback: the planes are integrated only in librsp.so.
"""
import ctypes as C

import numpy as np

from . import _capi as capi


def walk_shifts(v_scale, dt, delta_r, n, rate_sign=1.0):
    """int32 [n-1][V]: the columns a target of Doppler row v moves in i = 1 .. n-1 CPIs,
    np.rint(i * rate_sign * v_scale * dt / delta_r) in fp64 (half-way cases round to even).  v_scale
    [V] is the velocity of each row, dt the seconds between CPIs, delta_r the range cell; the sign
    convention is the tracker's: range moves by rate_sign * v * dt."""
    v = np.asarray(v_scale, dtype=np.float64).reshape(-1)
    i = np.arange(1, int(n), dtype=np.float64)[:, None]
    return np.rint(i * float(rate_sign) * v[None, :] * float(dt) / float(delta_r)).astype(np.int32).reshape(int(n) - 1, v.size)


class Integrator:
    """n: the CPI itself and the n-1 before it on its slot (1..16).  m=None: the sum form's parameters
    only; m = 1..n and spread = 0..2 columns are count_dev's.  Owns an rsp context (the CFAR-only kind),
    or borrows an Engine's; the history and meta tensors are allocated on first use for the window's
    (V, R) and dtype (one Integrator serves one form and one window shape at a time)."""

    def __init__(self, device=0, engine=None, n=4, slots=1, m=None, spread=0):
        import torch
        self.lib = capi.load_library()
        self.n, self.slots = int(n), int(slots)
        self.m, self.spread = (None if m is None else int(m)), int(spread)
        # refuse malformed parameters before anything is allocated: a well-formed call without a
        # context gets as far as "null ctx"
        for form in ("sum", "count") if m is not None else ("sum",):
            p = self._params(form, 1, 1)
            fn = self.lib.rsp_integrate_dev if form == "sum" else self.lib.rsp_binint_dev
            rc = fn(None, 1 << 40, 1, 1, 0, C.byref(p), None, None, self.slots, 2 << 40, 3 << 40, 4 << 40, None, None)
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
        self.hist = None
        self.meta = torch.zeros((self.slots, 2), dtype=torch.int32, device=self.device)
        self._shape = None

    def _params(self, form, ld, cs):
        p = capi.rsp_integ_params()
        p.n, p.reserved, p.ld, p.cpi_stride = self.n, 0, int(ld), int(cs)
        p.m, p.spread = (0, 0) if form == "sum" else (self.m, self.spread)
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

    def reset(self):
        """Forget every slot's history (meta is zeroed; the rings need no clearing)."""
        self.meta.zero_()

    def _run(self, form, planes, shift, slot, cols, out, stream):
        import torch
        who = "sum_dev" if form == "sum" else "count_dev"
        dtype = torch.float32 if form == "sum" else torch.uint8
        esz = 4 if form == "sum" else 1
        if form == "count" and self.m is None:
            raise ValueError("count_dev: the Integrator was made without m")
        if isinstance(planes, torch.Tensor):
            a = planes.to(self.device, dtype).contiguous()
        else:
            a = torch.as_tensor(np.ascontiguousarray(planes), device=self.device).to(dtype).contiguous()
        if a.dim() == 2:
            a = a[None]
        if a.dim() != 3:
            raise ValueError("%s: planes %s must be [batch][V][R]" % (who, tuple(a.shape)))
        B, V, Rp = a.shape
        lo, hi = (0, Rp) if cols is None else (int(cols[0]), int(cols[1]))
        if not 0 <= lo < hi <= Rp:
            raise ValueError("%s: column window %r outside 0..%d" % (who, (lo, hi), Rp))
        R = hi - lo
        if out is None:
            out = (torch.empty if cols is None else torch.zeros)((B, V, Rp), dtype=dtype, device=self.device)
        elif (tuple(out.shape) != (B, V, Rp) or out.dtype != dtype or not out.is_contiguous() or out.device != a.device):
            raise ValueError("%s: out must be a contiguous %s tensor of shape %s on %s" % (who, dtype, (B, V, Rp), a.device))
        key = (form, V, R)
        if self._shape != key:
            if self._shape is not None and int(self.meta[:, 0].max().item()) != 0:
                raise ValueError("%s: the history holds %s planes of %d x %d; reset() before changing the window or the form"
                                 % (who, self._shape[0], self._shape[1], self._shape[2]))
            self.hist = torch.empty((self.slots, max(self.n - 1, 0), V, R), dtype=dtype, device=self.device)
            self._shape = key
        if shift is None:
            sh = None
        else:
            if isinstance(shift, torch.Tensor):
                sh = shift.to(self.device, torch.int32).contiguous()
            else:
                sh = torch.as_tensor(np.ascontiguousarray(np.asarray(shift, dtype=np.int32)), device=self.device)
            if tuple(sh.shape) != (self.n - 1, V):
                raise ValueError("%s: shift %s must be [n-1 = %d][V = %d]" % (who, tuple(sh.shape), self.n - 1, V))
        if slot is None or isinstance(slot, int):
            sl = None if not slot else torch.full((B,), int(slot), dtype=torch.int32, device=self.device)
        elif isinstance(slot, torch.Tensor):
            sl = slot.to(self.device, torch.int32).contiguous()
        else:
            sl = torch.as_tensor(np.asarray(slot, dtype=np.int32), device=self.device)
        if sl is not None and tuple(sl.shape) != (B,):
            raise ValueError("%s: slot must hold one entry per CPI" % who)
        neff = torch.empty((B,), dtype=torch.int32, device=self.device)
        p = self._params(form, Rp, V * Rp)
        st = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None   # noqa: E731
        fn = self.lib.rsp_integrate_dev if form == "sum" else self.lib.rsp_binint_dev
        capi.check(fn(self.ctx, a.data_ptr() + esz * lo, V, R, B, C.byref(p), ptr(sh), ptr(sl), self.slots,
                      ptr(self.hist), self.meta.data_ptr(), out.data_ptr() + esz * lo, ptr(neff), C.c_void_p(st)), self.ctx)
        self._keep = (a, sh, sl)    # alive until the caller synchronises
        return out, neff

    def sum_dev(self, planes, shift=None, slot=None, cols=None, out=None, stream=None):
        """planes float32 [batch][V][Rp] (amplitudes; a device tensor, or an array copied to the
        device), consecutive CPIs in batch order.  shift: int32 [n-1][V] (walk_shifts) or None (no
        walk).  slot: None (all slot 0), an int, or int32 [batch]; a CPI whose slot is negative or
        >= slots touches no state and comes out as it went in.  cols = (lo, hi) takes the column
        window lo..hi-1 of every plane in place, as OsCfar.detect_dev does: nothing is shifted across
        its edges, and columns of `out` outside it keep their bytes (a new tensor is zeroed there).
        out must not be planes.  Returns (out, neff): the integrated planes and int32 [batch], the
        planes each sum holds.  Asynchronous on `stream` (default: torch's current stream)."""
        return self._run("sum", planes, shift, slot, cols, out, stream)

    def count_dev(self, flags, shift=None, slot=None, cols=None, out=None, stream=None):
        """The binary form over uint8 flag planes: out is 1 where at least m of the last n CPIs have
        a hit (the CPI itself in the cell; a past CPI within `spread` columns of the walked-back
        cell).  Arguments and returns as sum_dev's."""
        return self._run("count", flags, shift, slot, cols, out, stream)


def detector(integ, shift=None, inner=None):
    """A callable (rdm, flag, cfar) for rsp.score.sweep / scr_sweep's `detector`: the Integrator is
    reset, the batch is integrated as consecutive CPIs of slot 0 (sum_dev with `shift`) and `inner`,
    a callable (rdm, flag, cfar), runs on the result; inner defaults to the cfar_dev of the Engine the
    Integrator was made with."""
    if inner is None:
        if integ._engine is None:
            raise ValueError("detector: give inner=, or make the Integrator with engine=")
        eng = integ._engine

        def inner(rdm, flag, cfar):
            eng.cfar_dev(rdm, flag, cfar=cfar)

    def run(rdm, flag, cfar):
        integ.reset()
        acc, _ = integ.sum_dev(rdm, shift=shift)
        inner(acc, flag, cfar)
    return run
