"""Plots joined into tracks from CPI to CPI, through rsp_track_dev
(csrc/rsp_track.hip).

The chain ends at a per-CPI list of estimates {rEst, vEst, eleAngleEst} (Measure.measure_dev).  The
Tracker says which estimates of successive CPIs are one target, smooths them and throws away false
alarms that do not repeat: gated nearest-neighbour association with fixed gains, M-of-N
confirmation, deletion after consecutive misses (include/rsp.h states every step).  The state stays
on the device, `slots` independent track tables of max_tracks entries:

    state_f float64 [slots][max_tracks][4] = {r, v, ele, 0}
    state_i int32   [slots][max_tracks][8] = {id, status, hist, misses, hits, age, last_plot, 0}
    meta    int32   [slots][2]             = {next_id, cpis}

No CPU fallback: the association runs only in librsp.so.
"""
import ctypes as C

import numpy as np

from . import _capi as capi

FREE, TENTATIVE, CONFIRMED = 0, 1, 2


class Tracker:
    """gate = (gate_r, gate_v) in the units of rEst / vEst, alpha = (alpha_r, alpha_v, alpha_e) the
    smoothing gains in (0, 1], confirm = (M, N), drop = (consecutive misses that delete a tentative
    track, a confirmed one), dt the seconds between consecutive CPIs of a slot, rate_sign +1 or -1:
    range moves by rate_sign * v * dt."""

    def __init__(self, device=0, slots=1, max_tracks=256, confirm=(3, 5), drop=(2, 4), dt=None, rate_sign=1.0,
                 gate=None, alpha=(0.5, 0.5, 0.5)):
        import torch
        if dt is None or gate is None:
            raise ValueError("Tracker: give dt and gate=(gate_r, gate_v)")
        p = capi.rsp_track_params()
        p.max_tracks, p.confirm_m, p.confirm_n = int(max_tracks), int(confirm[0]), int(confirm[1])
        p.drop_tentative, p.drop_confirmed, p.reserved = int(drop[0]), int(drop[1]), 0
        p.dt, p.rate_sign = float(dt), float(rate_sign)
        p.gate_r, p.gate_v = float(gate[0]), float(gate[1])
        p.alpha_r, p.alpha_v, p.alpha_e = (float(x) for x in alpha)
        self.params = p
        self.slots, self.max_tracks = int(slots), int(max_tracks)
        self.lib = capi.load_library()
        # refuse malformed parameters before anything is allocated: a well-formed call without a
        # context gets as far as "null ctx"
        rc = self.lib.rsp_track_dev(None, None, 1 << 40, 0, 0, C.byref(p), None, None, self.slots, 2 << 40, 3 << 40,
                                    4 << 40, None, None, None, 5 << 40, None)
        msg = (self.lib.rsp_last_error(None) or b"").decode()
        if "null ctx" not in msg:
            raise capi.RspError(rc, msg)
        self.device = torch.device("cuda", device)
        ctx = C.c_void_p()
        capi.check(self.lib.rsp_create(C.byref(ctx), int(device), None), None)
        self.ctx = ctx
        T = self.max_tracks
        self.state_f = torch.zeros((self.slots, T, 4), dtype=torch.float64, device=self.device)
        self.state_i = torch.zeros((self.slots, T, 8), dtype=torch.int32, device=self.device)
        self.meta = torch.zeros((self.slots, 2), dtype=torch.int32, device=self.device)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.rsp_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update_dev(self, est, count, slot=None, dt=None, snapshot=True, stream=None):
        """est: contiguous CUDA float64 [batch, max_hits, 3], count: contiguous CUDA int32 [batch, 2]
        (Measure.measure_dev's outputs); the CPIs are consecutive in time and are applied in order.
        slot: None (all slot 0), an int, or int32 [batch] (a device tensor, or a sequence copied to
        the device); a CPI whose slot is negative or >= slots touches no state.  dt: None (the
        Tracker's), or float64 [batch], the time since the slot's previous CPI.  Returns (assign
        int32 [batch, max_hits], snap_f float64 [batch, max_tracks, 4], snap_i int32
        [batch, max_tracks, 8], tcount int32 [batch, 8]): the id each plot updated or started (0
        none, -1 an invalid plot), the slot's state after each CPI (None, None with
        snapshot=False) and {live, confirmed, started, dropped, not_started, n_valid, matched, 0}.
        Asynchronous on `stream` (default: torch's current stream)."""
        import torch
        if not isinstance(est, torch.Tensor) or not est.is_cuda or not est.is_contiguous() or est.dtype != torch.float64 \
                or est.dim() != 3 or est.shape[2] != 3:
            raise ValueError("est must be a contiguous CUDA float64 tensor [batch, max_hits, 3]")
        batch, max_hits = int(est.shape[0]), int(est.shape[1])
        if not isinstance(count, torch.Tensor) or not count.is_cuda or not count.is_contiguous() \
                or count.dtype != torch.int32 or tuple(count.shape) != (batch, 2):
            raise ValueError("count must be a contiguous CUDA int32 tensor [batch, 2]")
        if slot is None or isinstance(slot, int):
            sl = None if not slot else torch.full((batch,), int(slot), dtype=torch.int32, device=self.device)
        elif isinstance(slot, torch.Tensor):
            sl = slot.to(self.device, torch.int32).contiguous()
        else:
            sl = torch.as_tensor(np.asarray(slot, dtype=np.int32), device=self.device)
        if sl is not None and tuple(sl.shape) != (batch,):
            raise ValueError("slot must hold one entry per CPI")
        if dt is None:
            dts = None
        elif isinstance(dt, torch.Tensor):
            dts = dt.to(self.device, torch.float64).contiguous()
        else:
            dts = torch.as_tensor(np.asarray(dt, dtype=np.float64), device=self.device)
        if dts is not None and tuple(dts.shape) != (batch,):
            raise ValueError("dt must hold one entry per CPI")
        T = self.max_tracks
        assign = torch.empty((batch, max_hits), dtype=torch.int32, device=self.device)
        snap_f = torch.empty((batch, T, 4), dtype=torch.float64, device=self.device) if snapshot else None
        snap_i = torch.empty((batch, T, 8), dtype=torch.int32, device=self.device) if snapshot else None
        tcount = torch.empty((batch, 8), dtype=torch.int32, device=self.device)
        st = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None   # noqa: E731
        capi.check(self.lib.rsp_track_dev(
            self.ctx, ptr(est), count.data_ptr() if batch else self.meta.data_ptr(), max_hits, batch,
            C.byref(self.params), ptr(sl), ptr(dts), self.slots, self.state_f.data_ptr(), self.state_i.data_ptr(),
            self.meta.data_ptr(), ptr(assign), ptr(snap_f), ptr(snap_i),
            tcount.data_ptr() if batch else self.meta.data_ptr(), C.c_void_p(st)), self.ctx)
        self._keep = (est, count, sl, dts)    # alive until the caller synchronises
        return assign, snap_f, snap_i, tcount

    def reset(self, slot=None):
        """Forget a slot's tracks and its id counter (all slots by default)."""
        for t in (self.state_f, self.state_i, self.meta):
            if slot is None:
                t.zero_()
            else:
                t[int(slot)].zero_()

    def state(self):
        """(state_f, state_i, meta) as new tensors: what load_state takes back."""
        return self.state_f.clone(), self.state_i.clone(), self.meta.clone()

    def load_state(self, state):
        for mine, theirs in zip((self.state_f, self.state_i, self.meta), state):
            if tuple(mine.shape) != tuple(theirs.shape):
                raise ValueError("load_state: %s does not fit %s" % (tuple(theirs.shape), tuple(mine.shape)))
            mine.copy_(theirs)

    def confirmed(self, slot=0):
        """The confirmed tracks of a slot on the host (synchronises): a dict of arrays id, r, v,
        ele, hits, age, in entry order."""
        sf = self.state_f[int(slot)].cpu().numpy()
        si = self.state_i[int(slot)].cpu().numpy()
        k = np.flatnonzero(si[:, 1] == CONFIRMED)
        return dict(id=si[k, 0].copy(), r=sf[k, 0].copy(), v=sf[k, 1].copy(), ele=sf[k, 2].copy(), hits=si[k, 4].copy(),
                    age=si[k, 5].copy())
