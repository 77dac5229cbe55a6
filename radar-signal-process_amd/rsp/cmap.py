"""Clutter-map detection in the zero-velocity band the chain blanks, through
rsp_cmap_dev (csrc/rsp_cmap.hip).

The MTD writes zeros over the Doppler rows round zero velocity and the CFAR strips them: a
hovering target is invisible there by construction.  ClutterMap computes those rows' bins from the
pulse-compressed rows (Engine.pc_dev's output, the same tensor Engine.mtd_dev takes), keeps a
recursive average of every band cell over CPIs and flags a cell that stands over its own history:

    flag = age >= max(warmup, 1) and a >= T * m
    m'   = a                 on a slot's first CPI
    m'   = m                 where hold and flag
    m'   = m + w * (a - m)   otherwise

  * band_of(spec, cfar=None) -> (q_lo, q_hi): the signed DFT bins of the rows a spec's chain zeroes.
  * rows(q_lo, q_hi, V, fftshift): the RDM row of each bin.
  * ClutterMap: owns the map and age tensors; update_dev(pc) -> (band, flag); merge_flags writes
    the band flags into the band's rows of a chain flag plane.

No CPU fallback: the band and the recursion are computed only in librsp.so.
"""
import ctypes as C

import numpy as np

from . import _capi as capi


def _mround(x):
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


def zero_v_bins(V, div):
    """fun_0v_pressing's rows of an fftshifted RDM of V rows, round(V/2) - round(V/div) - 1 ..
    round(V/2) + round(V/div) - 1 (0-based), as bins: row = (q + V // 2) % V.  P = 128, /150:
    bins -2..0, off-centre as the reference is."""
    zv, k = _mround(V / 2.0), _mround(V / float(div))
    return zv - k - 1 - V // 2, zv + k - 1 - V // 2


def band_of(spec, cfar=None):
    """(q_lo, q_hi) of the rows the spec's chain zeroes: zero_ends = n zeroes rows [0, n) and
    [V - n + 1, V) of an unshifted RDM, bins -(n - 1)..n - 1; otherwise zero_v_div's rows of the
    fftshifted RDM.  With cfar (a presets.Cfar) the band is widened to the rows the CFAR blanks
    round zero velocity as well: its own zero_v_div band (main_cfar's /20) on an fftshifted RDM,
    and executeCFAR's strip of rows 0..M0 and V-M0..V-1 on an unshifted one (bins -M0..M0; on an
    fftshifted RDM that strip lies at the folding velocity, not in this band)."""
    V = spec.V
    bands = []
    if spec.zero_ends > 0:
        if spec.fftshift:
            raise ValueError("band_of: zero_ends on an fftshifted RDM is not a band round zero velocity")
        bands.append((-(spec.zero_ends - 1), spec.zero_ends - 1))
    elif spec.zero_v_div:
        if not spec.fftshift:
            raise ValueError("band_of: zero_v_div on an unshifted RDM is not a band round zero velocity")
        bands.append(zero_v_bins(V, spec.zero_v_div))
    if cfar is not None:
        if cfar.zero_v_div and spec.fftshift:
            bands.append(zero_v_bins(V, cfar.zero_v_div))
        if not spec.fftshift:
            bands.append((-cfar.M0, cfar.M0))
    if not bands:
        raise ValueError("band_of: the chain zeroes no rows")
    return min(b[0] for b in bands), max(b[1] for b in bands)


def rows(q_lo, q_hi, V, fftshift):
    """The RDM row of each bin q_lo..q_hi (int64 [K])."""
    q = np.arange(int(q_lo), int(q_hi) + 1, dtype=np.int64)
    return (q + V // 2) % V if fftshift else q % V


class ClutterMap:
    """The map of one band: `slots` independent maps (beam positions, scan sectors) of K x R cells
    and their ages, as device tensors `map` float32 [slots, K, R] and `age` int32 [slots].

    Either spec (a presets.Spec: P, V, beams, window, fftshift and, unless band is given,
    band_of(spec, cfar)) or the explicit fields P, V, beams, window, window_beta, band, fftshift."""

    def __init__(self, spec=None, R=None, slots=1, T=4.0, w=0.125, warmup=4, hold=True, device=0, cfar=None,
                 band=None, P=None, V=0, beams=1, window=capi.RSP_WIN_KAISER, window_beta=8.0, fftshift=1):
        import torch
        if spec is not None:
            P, V, beams, window, window_beta = spec.P, spec.V, spec.beams, spec.window, spec.window_beta
            fftshift = spec.fftshift
            if R is None:
                R = spec.R_out
            if band is None:
                band = band_of(spec, cfar)
        if P is None or R is None or band is None:
            raise ValueError("ClutterMap: give a spec, or P, R and band")
        self.P, self.V, self.R, self.beams = int(P), int(V) or int(P), int(R), int(beams)
        self.window, self.window_beta, self.fftshift = int(window), float(window_beta), int(fftshift)
        self.q_lo, self.q_hi = int(band[0]), int(band[1])
        self.K = self.q_hi - self.q_lo + 1
        self.slots, self.T, self.w, self.warmup, self.hold = int(slots), float(T), float(w), int(warmup), bool(hold)
        self.lib = capi.load_library()
        # refuse a malformed band before anything is allocated (rsp_cmap_plan checks all of it)
        self.plan(1)
        self.device = torch.device("cuda", device)
        ctx = C.c_void_p()
        capi.check(self.lib.rsp_create(C.byref(ctx), int(device), None), None)
        self.ctx = ctx
        self.map = torch.zeros((self.slots, self.K, self.R), dtype=torch.float32, device=self.device)
        self.age = torch.zeros((self.slots,), dtype=torch.int32, device=self.device)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.rsp_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _params(self, ld=0, cpi_stride=0):
        p = capi.rsp_cmap_params()
        p.P, p.V, p.beams, p.window, p.window_beta = self.P, self.V, self.beams, self.window, self.window_beta
        p.q_lo, p.q_hi, p.warmup, p.hold, p.T, p.w = self.q_lo, self.q_hi, self.warmup, int(self.hold), self.T, self.w
        p.ld, p.cpi_stride = int(ld), int(cpi_stride)
        return p

    def plan(self, batch=1, ld=0, cpi_stride=0):
        """The band kernel instance a call takes, as a dict of rsp_cmap_plan_t's fields."""
        out = capi.rsp_cmap_plan_t()
        p = self._params(ld, cpi_stride)
        capi.check(self.lib.rsp_cmap_plan(None, self.R, int(batch), C.byref(p), C.byref(out)), None)
        return {n: getattr(out, n) for n, _ in out._fields_ if n != "reserved"}

    def rows(self):
        """The RDM row of each band bin."""
        return rows(self.q_lo, self.q_hi, self.V, self.fftshift)

    def update_dev(self, pc, slot=None, stream=None, batch=None, ld=0, cpi_stride=0, band=True):
        """pc: contiguous CUDA complex64 [batch, (beams,) P, R] (Engine.pc_dev's output); the CPIs
        are consecutive in time and are applied in order.  slot: None (all slot 0), an int, or
        int32 [batch] (a device tensor, or a sequence copied to the device); a negative slot's CPI
        gets its amplitudes and zero flags and updates nothing.  batch / ld / cpi_stride describe
        other layouts of pc's memory (a padded pitch, overlapping CPIs of a window stream): pc is
        then any contiguous complex64 tensor that holds them.  Returns (band float32
        [batch, K, R] or None with band=False, flag uint8 [batch, K, R]); asynchronous on
        `stream` (default: torch's current stream)."""
        import torch
        if not isinstance(pc, torch.Tensor) or not pc.is_cuda or not pc.is_contiguous() or pc.dtype != torch.complex64:
            raise ValueError("pc must be a contiguous CUDA complex64 tensor")
        if batch is None:
            want = (self.P, self.R) if self.beams == 1 else (self.beams, self.P, self.R)
            if tuple(pc.shape[1:]) != want:
                raise ValueError("pc is %s, the map expects [batch, %s]" % (tuple(pc.shape), want))
            batch = pc.shape[0]
        else:
            pitch = int(ld) or self.R
            cs = int(cpi_stride) or self.beams * self.P * pitch
            if batch > 0 and (batch - 1) * cs + (self.beams * self.P - 1) * pitch + self.R > pc.numel():
                raise ValueError("pc holds %d elements, too few for %d CPIs of this layout" % (pc.numel(), batch))
        batch = int(batch)
        if slot is None or isinstance(slot, int):
            sl = None if not slot else torch.full((batch,), int(slot), dtype=torch.int32, device=self.device)
        elif isinstance(slot, torch.Tensor):
            sl = slot.to(self.device, torch.int32).contiguous()
        else:
            sl = torch.as_tensor(np.asarray(slot, dtype=np.int32), device=self.device)
        if sl is not None and tuple(sl.shape) != (batch,):
            raise ValueError("slot must hold one entry per CPI")
        out_band = torch.empty((batch, self.K, self.R), dtype=torch.float32, device=self.device) if band else None
        flag = torch.empty((batch, self.K, self.R), dtype=torch.uint8, device=self.device)
        p = self._params(ld, cpi_stride)
        st = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.rsp_cmap_dev(
            self.ctx, pc.data_ptr(), self.R, batch, C.byref(p), sl.data_ptr() if sl is not None else None,
            self.slots, self.map.data_ptr(), self.age.data_ptr(),
            out_band.data_ptr() if out_band is not None else None, flag.data_ptr(), C.c_void_p(st)), self.ctx)
        self._keep = (pc, sl)    # alive until the caller synchronises
        return out_band, flag

    def reset(self, slot=None):
        """Forget a slot's history (all slots by default): its next CPI initialises the map."""
        if slot is None:
            self.age.zero_()
        else:
            self.age[int(slot)] = 0

    def state(self):
        """(map, age) as new tensors: what load_state takes back."""
        return self.map.clone(), self.age.clone()

    def load_state(self, state):
        m, a = state
        if tuple(m.shape) != tuple(self.map.shape) or tuple(a.shape) != tuple(self.age.shape):
            raise ValueError("load_state: map %s / age %s do not fit %s / %s"
                             % (tuple(m.shape), tuple(a.shape), tuple(self.map.shape), tuple(self.age.shape)))
        self.map.copy_(m)
        self.age.copy_(a)

    def merge_flags(self, flag_plane, band_flag):
        """Write band_flag [batch, K, R] into the band's rows of a chain flag plane
        [batch, V, R] (in place; the rows the chain leaves zero).  Returns flag_plane."""
        import torch
        idx = torch.as_tensor(self.rows(), device=flag_plane.device)
        flag_plane[:, idx, :] = band_flag.to(flag_plane.dtype)
        return flag_plane
