"""CFAR detections scored against truth on the GPU: the evaluation functions at the end of
MatlabProcess_xuzerui/CFAR_WangCai/main_cfar.m (:163-279), the reason for its `for T=[5]`
threshold loop (:40), with the reference's names and argument meaning:

  * fun_frame_fa(cfarFlag, R_True, V_True, R_True_index, V_True_index) -> fa          (:163-175)
  * fun_drate(cfarFlag_all, R, V, r_axis, v_axis, frameRInds) -> drate                (:177-206)
  * fun_accuracy(cfarFlag_all, R, V, r_axis, v_axis, frameRInds) -> acc               (:208-234)
  * fun_PCF(cfarFlag_all, R, V, r_axis, v_axis, frameRInds, MTD_data_all) -> pof      (:236-279)
    Indices are MATLAB's (1-based) in these four, as in the reference; where the reference
    stops with an index error they raise IndexError, and fun_PCF raises ValueError when the
    local maximum occurs more than once in the matrix (dv^2 of a vector, :265).
  * Scorer.score_dev(flag, rdm, truth_idx, params, cols=None, rows=None): the batched device
    form -- one 8-int record per CPI (include/rsp.h, rsp_score_dev), computed by
    csrc/rsp_score.hip where the flags and the RDM already are.
  * Scorer.summary(rec, truth_idx, V, R, params): the records -> fa per CPI, drate, acc, pof and
    the counters (rsp_score_summary, host arithmetic in the reference's order).
  * truth_index(r_axis, v_axis, R_true, V_true): the find(min(abs(axis - x)) == ...) lookups of
    :183-184 (first bin of a tie) and the validity gate, 0-based.
  * sweep(engine, echo_dev, truth_idx, T_values, cfar): main_cfar.m:40-58's threshold loop on a
    device-resident batch; only the batch x 8 records cross PCIe.
  * scr_sweep(engine, clutter_dev, plan, SCR_values, cfar, seg): the Pd-versus-SCR loop: for
    each SCR the plan's targets are injected into the clutter on the device (rsp.inject), the
    chain and the CFAR run, and the flags are scored against the plan's truth cells.
    Both sweeps take detector=, a callable in place of the chain's CFAR (rsp.oscfar.detector).

Quirks of the reference kept as they are: `for i=1:length(cfarFlag_all)` is the largest
dimension of the 3-D array (here the loop runs over the batch, the first dimension), and
fun_accuracy counts a frame without a valid truth when it holds any flag at all (:224-227).

No CPU fallback: the records are computed only in librsp.so.
"""
import ctypes as C
import dataclasses

import numpy as np

from . import _capi as capi

REC_FIELDS = ("n_flags", "n_box", "box_status", "n_pcf", "pcf_status", "n_peak", "peak_v", "peak_r")
GATE = (3, 20, 400, 2000)   # abs(V) > 3 && abs(V) < 20 && R > 400 && R < 2000 (:165)


def score_params(hv=3, hr=7, n_cell=20, v_lim=155, r_lim=288):
    """rsp_score_params with the reference's constants: the +-3 x +-7 detection box (:167),
    fun_PCF's n_cell = 20 (:247) and the limits 155 / 288 its elseif chain compares with
    (:250-255, the size of the clipped dataset matrices)."""
    p = capi.rsp_score_params()
    p.hv, p.hr, p.n_cell, p.v_lim, p.r_lim = int(hv), int(hr), int(n_cell), int(v_lim), int(r_lim)
    return p


def truth_index(r_axis, v_axis, R_true, V_true, gate=GATE):
    """int32 [batch][3] = {v_idx, r_idx, valid}, 0-based: the nearest axis bins as
    find(min(abs(axis - x)) == abs(axis - x)) gives them (:183-184; the first bin of a tie,
    which is what the colon of the box takes) and the validity gate
    abs(V) > gate[0] && abs(V) < gate[1] && R > gate[2] && R < gate[3]."""
    r_axis = np.asarray(r_axis, np.float64).reshape(-1)
    v_axis = np.asarray(v_axis, np.float64).reshape(-1)
    Rt = np.atleast_1d(np.asarray(R_true, np.float64))
    Vt = np.atleast_1d(np.asarray(V_true, np.float64))
    if Rt.shape != Vt.shape or Rt.ndim != 1:
        raise ValueError("truth_index: R_true %s and V_true %s must be vectors of one length" % (Rt.shape, Vt.shape))
    out = np.empty((Rt.size, 3), np.int32)
    for i in range(Rt.size):
        out[i, 0] = int(np.argmin(np.abs(v_axis - Vt[i])))   # argmin: the first minimum
        out[i, 1] = int(np.argmin(np.abs(r_axis - Rt[i])))
        out[i, 2] = int(gate[0] < abs(Vt[i]) < gate[1] and gate[2] < Rt[i] < gate[3])
    return out


class Scorer:
    """rsp_score_dev on a context of its own (the CFAR-only kind) or on an Engine's."""

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

    params = staticmethod(score_params)

    def _dev(self, x, dtype):
        import torch
        if isinstance(x, torch.Tensor):
            return x.to(self.device, dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(x), device=self.device).to(dtype).contiguous()

    def score_dev(self, flag, rdm, truth_idx, params, cols=None, rows=None, stream=None):
        """flag uint8 [batch][Vp][Rp] (values 0/1), rdm float32 of the same shape or None (no
        fun_PCF peak search), truth_idx int32 [batch][3] = {v_idx, r_idx, valid} (truth_index);
        device tensors, or arrays copied to the device.  rows = (lo, hi) / cols = (lo, hi) score
        the window rows lo..hi-1, columns lo..hi-1 of every plane in place (clip.m:12's rows
        691:845 of a 1536-row RDM are rows=(690, 845)); the truth indices are relative to the
        window.  Returns the records, int32 [batch][8] (REC_FIELDS), on the device;
        asynchronous on `stream` (default: torch's current stream)."""
        import torch
        f = self._dev(flag, torch.uint8)
        d = self._dev(rdm, torch.float32) if rdm is not None else None
        if f.dim() == 2:
            f = f[None]
            d = d[None] if d is not None else None
        if f.dim() != 3 or (d is not None and d.shape != f.shape):
            raise ValueError("score_dev: flag %s and rdm %s must be [batch][V][R] of one shape"
                             % (tuple(f.shape), None if d is None else tuple(d.shape)))
        B, Vp, Rp = f.shape
        r_lo, r_hi = (0, Vp) if rows is None else (int(rows[0]), int(rows[1]))
        c_lo, c_hi = (0, Rp) if cols is None else (int(cols[0]), int(cols[1]))
        if not 0 <= r_lo < r_hi <= Vp or not 0 <= c_lo < c_hi <= Rp:
            raise ValueError("score_dev: window rows %r x columns %r outside %d x %d"
                             % ((r_lo, r_hi), (c_lo, c_hi), Vp, Rp))
        t = self._dev(np.asarray(truth_idx) if not isinstance(truth_idx, torch.Tensor) else truth_idx, torch.int32)
        if tuple(t.shape) != (B, 3):
            raise ValueError("score_dev: truth_idx is %s, expected (%d, 3)" % (tuple(t.shape), B))
        p = capi.rsp_score_params()
        C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        p.ld, p.cpi_stride = Rp, Vp * Rp
        off = r_lo * Rp + c_lo
        rec = torch.empty((B, 8), dtype=torch.int32, device=self.device)
        st = stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.rsp_score_dev(
            self.ctx, f.data_ptr() + off, (d.data_ptr() + 4 * off) if d is not None else None, r_hi - r_lo,
            c_hi - c_lo, B, C.byref(p), t.data_ptr(), rec.data_ptr(), C.c_void_p(st)), self.ctx)
        self._keep = (f, d, t)    # alive until the caller synchronises
        return rec

    def summary(self, rec, truth_idx, V, R, params):
        """rsp_score_summary on host copies of the records (synchronises when rec is a device
        tensor): dict(fa float64 [batch], drate, acc, pof, n_valid, n_scored, n_index_error
        {function: count}, n_multi_peak)."""
        return summary(rec, truth_idx, V, R, params, lib=self.lib)

    # ---- the reference's own functions -----------------------------------------------------
    def _records(self, cfarFlag_all, truth, MTD_data_all=None):
        import torch
        fl = cfarFlag_all
        fl = (fl != 0).to(torch.uint8) if isinstance(fl, torch.Tensor) else (np.asarray(fl) != 0).astype(np.uint8)
        if fl.ndim == 2:
            fl = fl[None]
            if MTD_data_all is not None and MTD_data_all.ndim == 2:
                MTD_data_all = MTD_data_all[None]
        p = score_params()
        rec = self.score_dev(fl, MTD_data_all, truth, p).cpu().numpy()
        return rec, p, fl.shape[1], fl.shape[2]

    @staticmethod
    def _frames_truth(R, V, r_axis, v_axis, frameRInds):
        idx = np.asarray(frameRInds, np.int64).reshape(-1) - 1         # R(frameRInd): 1-based
        return truth_index(r_axis, v_axis, np.asarray(R, np.float64).reshape(-1)[idx],
                           np.asarray(V, np.float64).reshape(-1)[idx])

    @staticmethod
    def _stop(fn, n):
        if n:
            raise IndexError("%s: the truth box leaves the matrix at %d frame(s); the reference stops with an "
                             "index error there" % (fn, n))

    def fun_frame_fa(self, cfarFlag, R_True, V_True, R_True_index, V_True_index):  # noqa: N802,N803
        """main_cfar.m:163-175 for one V x R flag matrix; the indices are MATLAB's (1-based)."""
        valid = int(GATE[0] < abs(V_True) < GATE[1] and GATE[2] < R_True < GATE[3])
        truth = np.array([[int(V_True_index) - 1, int(R_True_index) - 1, valid]], np.int32)
        rec, p, V, R = self._records(cfarFlag, truth)
        s = summary(rec, truth, V, R, p, lib=self.lib)
        self._stop("fun_frame_fa", s["n_index_error"]["fa"])
        return float(s["fa"][0])

    def fun_drate(self, cfarFlag_all, R, V, r_axis, v_axis, frameRInds):  # noqa: N802,N803
        """main_cfar.m:177-206; cfarFlag_all is [frames][V][R] and the loop runs over the frames."""
        truth = self._frames_truth(R, V, r_axis, v_axis, frameRInds)
        rec, p, nv, nr = self._records(cfarFlag_all, truth)
        s = summary(rec, truth, nv, nr, p, lib=self.lib)
        self._stop("fun_drate", s["n_index_error"]["drate"])
        return s["drate"]

    def fun_accuracy(self, cfarFlag_all, R, V, r_axis, v_axis, frameRInds):  # noqa: N802,N803
        """main_cfar.m:208-234, with its count of any-flag frames among the invalid truths."""
        truth = self._frames_truth(R, V, r_axis, v_axis, frameRInds)
        rec, p, nv, nr = self._records(cfarFlag_all, truth)
        s = summary(rec, truth, nv, nr, p, lib=self.lib)
        self._stop("fun_accuracy", s["n_index_error"]["acc"])
        return s["acc"]

    def fun_PCF(self, cfarFlag_all, R, V, r_axis, v_axis, frameRInds, MTD_data_all):  # noqa: N802,N803
        """main_cfar.m:236-279 (the limits 155 / 288 of its elseif chain included)."""
        truth = self._frames_truth(R, V, r_axis, v_axis, frameRInds)
        rec, p, nv, nr = self._records(cfarFlag_all, truth, MTD_data_all)
        s = summary(rec, truth, nv, nr, p, lib=self.lib)
        self._stop("fun_PCF", s["n_index_error"]["pcf"])
        if s["n_multi_peak"]:
            raise ValueError("fun_PCF: the local maximum occurs more than once in the matrix at %d frame(s); "
                             "dv^2 of a vector is a MATLAB error (main_cfar.m:265)" % s["n_multi_peak"])
        return s["pof"]


def summary(rec, truth_idx, V, R, params, lib=None):
    """rsp_score_summary (host only, no GPU): see Scorer.summary."""
    lib = lib or capi.load_library()
    if hasattr(rec, "cpu"):
        rec = rec.cpu().numpy()
    if hasattr(truth_idx, "cpu"):
        truth_idx = truth_idx.cpu().numpy()
    rec = np.ascontiguousarray(rec, np.int32)
    tr = np.ascontiguousarray(truth_idx, np.int32)
    B = rec.shape[0]
    if rec.shape != (B, 8) or tr.shape != (B, 3):
        raise ValueError("summary: rec %s / truth %s, expected (batch, 8) / (batch, 3)" % (rec.shape, tr.shape))
    fa = np.empty(B, np.float64)
    out = capi.rsp_score_result()
    capi.check(lib.rsp_score_summary(rec.ctypes.data, tr.ctypes.data, B, int(V), int(R), C.byref(params),
                                     fa.ctypes.data, C.byref(out)), None)
    return dict(fa=fa, drate=out.drate, acc=out.acc, pof=out.pof, n_valid=out.n_valid, n_scored=out.n_scored,
                n_index_error=dict(fa=out.n_index_error[capi.RSP_SCORE_FA], drate=out.n_index_error[capi.RSP_SCORE_DRATE],
                                   acc=out.n_index_error[capi.RSP_SCORE_ACC], pcf=out.n_index_error[capi.RSP_SCORE_PCF]),
                n_multi_peak=out.n_multi_peak)


def sweep(engine, echo_dev, truth_idx, T_values, cfar, params=None, on_step=None, detector=None):
    """The `for T=[...]` loop of main_cfar.m:40-58 on a device-resident echo batch: PC + MTD
    run once (the RDM does not depend on T); for each T the CFAR runs with TR = TV = T
    (T_CFAR_R = T_CFAR_V = T_CFAR, :47-53) through Engine.cfar_dev and the flags are scored
    where they are.  Only the batch x 8 records cross PCIe.  params: default the reference's
    box sizes with v_lim, r_lim = the RDM's own size.  on_step(T, flag, rdm, rec), if given,
    sees each step's device tensors (the same rdm object every time).  detector, if given, is a
    callable (rdm, flag, cfar) that fills flag from rdm with the step's cfar in place of
    Engine.cfar_dev (rsp.oscfar.detector: the ordered-statistic CFAR).  Returns
    [dict(T=T, **summary)] in the order of T_values."""
    import torch
    spec = engine.spec
    B = echo_dev.shape[0]
    V, R = spec.V, spec.R_out
    dev = echo_dev.device
    rdm = torch.empty((B, V, R), dtype=torch.float32, device=dev)
    flag = torch.empty((B, V, R), dtype=torch.uint8, device=dev)
    engine.run_dev(echo_dev, rdm=rdm)
    if params is None:
        params = score_params(v_lim=V, r_lim=R)
    scorer = Scorer(engine=engine)
    out = []
    for T in T_values:
        c = dataclasses.replace(cfar, TR=float(T), TV=float(T))
        if detector is None:
            engine.cfar_dev(rdm, flag, cfar=c)
        else:
            detector(rdm, flag, c)
        rec = scorer.score_dev(flag, rdm, truth_idx, params)
        if on_step is not None:
            on_step(T, flag, rdm, rec)
        out.append(dict(T=T, **summary(rec, truth_idx, V, R, params, lib=engine.lib)))
    return out


def scr_sweep(engine, clutter_dev, plan, SCR_values, cfar, seg=0, params=None, on_step=None, power=None,  # noqa: N803
              detector=None):
    """Detection scores over a sweep of signal-to-clutter ratios, everything in device memory:
    for each SCR [dB] the plan's point targets (rsp.inject.target_plan, one per CPI) are injected
    into clutter_dev ([K][P][R] complex64, K <= plan.batch) at that SCR into one reused buffer
    (rsp_inject_dev), the chain runs with `cfar` (Engine.run_dev) and the flags are scored against
    plan.truth_cells(spec, seg), the target in pulse-compression segment `seg`.  Only the batch x 8
    records cross PCIe.  params: default the reference's box sizes with v_lim, r_lim = the RDM's
    own size.  on_step(SCR, flag, rdm, rec), if given, sees each step's device tensors.  detector,
    if given, is a callable (rdm, flag, cfar): the chain then runs without its CFAR
    (run_dev(echo, rdm=rdm)) and the detector fills flag from rdm.  Returns
    [dict(SCR=SCR, **summary)] in the order of SCR_values."""
    import torch
    from . import inject
    spec = engine.spec
    B = plan.batch
    V, R = spec.V, spec.R_out
    dev = clutter_dev.device
    truth = plan.truth_cells(spec, seg)
    echo = torch.empty((B, spec.P, spec.R), dtype=torch.complex64, device=dev)
    rdm = torch.empty((B, V, R), dtype=torch.float32, device=dev)
    flag = torch.empty((B, V, R), dtype=torch.uint8, device=dev)
    if params is None:
        params = score_params(v_lim=V, r_lim=R)
    inj = inject.Injector(engine=engine)
    scorer = Scorer(engine=engine)
    out = []
    for scr in SCR_values:
        inj.inject_dev(clutter_dev, plan, float(scr), out=echo, power=inject.ABS2 if power is None else power)
        if detector is None:
            engine.run_dev(echo, rdm=rdm, flag=flag, cfar=cfar)
        else:
            engine.run_dev(echo, rdm=rdm)
            detector(rdm, flag, cfar)
        rec = scorer.score_dev(flag, rdm, truth, params)
        if on_step is not None:
            on_step(scr, flag, rdm, rec)
        out.append(dict(SCR=scr, **summary(rec, truth, V, R, params, lib=engine.lib)))
    return out
