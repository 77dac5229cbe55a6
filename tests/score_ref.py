"""fp64 restatement of the evaluation functions of MatlabProcess_xuzerui/CFAR_WangCai/
main_cfar.m:163-279 (fun_frame_fa, fun_drate, fun_accuracy, fun_PCF), loop for loop, in
MATLAB's 1-based index arithmetic on numpy arrays.  It raises IndexError where MATLAB stops
with an index error and ValueError where fun_PCF's dv^2 meets a vector (:265).

MATLAB semantics that matter here:
  * A(lo:hi, ...) READ: every index of a non-empty range must lie in 1..size, else an error;
    an empty range (hi < lo) is a valid index and gives an empty result, whose sum is 0.
  * A(lo:hi, ...) = 0 ASSIGNMENT: an index below 1 is an error; an index above the size grows
    the matrix with zeros.
  * find(x == A) lists matches in column-major order; NaN never matches.
  * `for i=1:length(A)` with a 3-D A runs to its LARGEST dimension (:179, :210, :238).  The
    batched restatement below loops over the frames (the first dimension), which is what the
    reference means and what it does whenever there are more frames than rows and columns.
  * find(min(abs(axis-x)) == abs(axis-x)) may return several bins on a tie; used in a colon
    expression only the first counts.

record() builds the 8-int per-CPI record of rsp_score_dev (include/rsp.h) out of the same
per-frame pieces.
"""
import math

import numpy as np

HV, HR, N_CELL, V_LIM, R_LIM = 3, 7, 20, 155, 288     # :167, :247, :250-255
DV_BASE, DR_BASE = 1 / 0.2719, 30 / 6                  # :237


def valid_truth(R_True, V_True):
    return (abs(V_True) > 3) and (abs(V_True) < 20) and (R_True > 400) and (R_True < 2000)    # :165


def nearest_index(axis, x):
    """find(min(abs(axis-x)) == abs(axis-x)), first element, 1-based."""
    d = np.abs(np.asarray(axis, np.float64) - x)
    return int(np.flatnonzero(d == d.min())[0]) + 1


def _check_range(lo, hi, size, what):
    if hi >= lo and (lo < 1 or hi > size):
        raise IndexError("%s %d:%d outside 1..%d" % (what, lo, hi, size))


def mread(A, vlo, vhi, rlo, rhi):
    """A(vlo:vhi, rlo:rhi) as a read."""
    m, n = A.shape
    _check_range(vlo, vhi, m, "rows")
    _check_range(rlo, rhi, n, "columns")
    if vhi < vlo or rhi < rlo:
        return A[0:0, 0:0]
    return A[vlo - 1:vhi, rlo - 1:rhi]


def massign_zero(A, vlo, vhi, rlo, rhi):
    """B = A; B(vlo:vhi, rlo:rhi) = 0 (grows B on the high side)."""
    m, n = A.shape
    if (vhi >= vlo and vlo < 1) or (rhi >= rlo and rlo < 1):
        raise IndexError("assignment index below 1")
    if vhi < vlo or rhi < rlo:
        return A.copy()
    B = np.zeros((max(m, vhi), max(n, rhi)), A.dtype)
    B[:m, :n] = A
    B[vlo - 1:vhi, rlo - 1:rhi] = 0
    return B


def fun_frame_fa(cfarFlag, R_True, V_True, R_True_index, V_True_index, hv=HV, hr=HR):
    cfarFlag = np.asarray(cfarFlag, np.float64)
    m, n = cfarFlag.shape                                                             # :164
    if valid_truth(R_True, V_True):
        temp = massign_zero(cfarFlag, V_True_index - hv, V_True_index + hv, R_True_index - hr, R_True_index + hr)
        n_p_1_0 = float(temp.sum())
        n_p_0_0 = m * n - n_p_1_0
    else:
        n_p_1_0 = float(cfarFlag.sum())
        n_p_0_0 = m * n - n_p_1_0
    return n_p_1_0 / (n_p_1_0 + n_p_0_0)                                              # :174


def _div(a, b):
    return a / b if b != 0 else math.nan       # MATLAB 0/0 (the numerators here are 0 then)


def _frames(cfarFlag_all, R, V, r_axis, v_axis, frameRInds):
    for i in range(1, np.shape(cfarFlag_all)[0] + 1):
        frameRInd = int(frameRInds[i - 1])
        R_True, V_True = float(R[frameRInd - 1]), float(V[frameRInd - 1])
        yield i, R_True, V_True, nearest_index(r_axis, R_True), nearest_index(v_axis, V_True)


def fun_drate(cfarFlag_all, R, V, r_axis, v_axis, frameRInds, hv=HV, hr=HR):
    n_p_1_1 = 0
    n_p_0_1 = 0
    for i, R_True, V_True, Ri, Vi in _frames(cfarFlag_all, R, V, r_axis, v_axis, frameRInds):
        cfarFlag = np.asarray(cfarFlag_all[i - 1], np.float64)
        if valid_truth(R_True, V_True):
            t = float(mread(cfarFlag, Vi - hv, Vi + hv, Ri - hr, Ri + hr).sum())      # :188
            if t > 0:
                n_p_1_1 += 1
            if t == 0:
                n_p_0_1 += 1
    return _div(n_p_1_1, n_p_1_1 + n_p_0_1)                                           # :205


def fun_accuracy(cfarFlag_all, R, V, r_axis, v_axis, frameRInds, hv=HV, hr=HR):
    n_p_1_1 = 0
    n_p_0_0 = 0
    N = np.shape(cfarFlag_all)[0]
    for i, R_True, V_True, Ri, Vi in _frames(cfarFlag_all, R, V, r_axis, v_axis, frameRInds):
        cfarFlag = np.asarray(cfarFlag_all[i - 1], np.float64)
        if valid_truth(R_True, V_True):
            t = float(mread(cfarFlag, Vi - hv, Vi + hv, Ri - hr, Ri + hr).sum())      # :219
            if t > 0:
                n_p_1_1 += 1
        else:
            t = float(cfarFlag.sum())                                                 # :224
            if t > 0:
                n_p_0_0 += 1
    return _div(n_p_1_1 + n_p_0_0, N)                                                 # :232


def pcf_ranges(Vi, Ri, n_cell=N_CELL, v_lim=V_LIM, r_lim=R_LIM):
    """(vlo, vhi, rlo, rhi) of the if / elseif chain at :248-258: one side clipped at most."""
    if Vi - n_cell < 1:
        return 1, Vi + n_cell, Ri - n_cell, Ri + n_cell
    elif Vi + n_cell > v_lim:
        return Vi - n_cell, v_lim, Ri - n_cell, Ri + n_cell
    elif Ri - n_cell < 1:
        return Vi - n_cell, Vi + n_cell, 1, Ri + n_cell
    elif Ri + n_cell > r_lim:
        return Vi - n_cell, Vi + n_cell, Ri - n_cell, r_lim
    return Vi - n_cell, Vi + n_cell, Ri - n_cell, Ri + n_cell


def pcf_frame(cfarFlag, MTD_data, Vi, Ri, n_cell=N_CELL, v_lim=V_LIM, r_lim=R_LIM):
    """:247-262 for one valid frame: (t, v_ind, r_ind) with the 1-based find() results in
    column-major order (empty lists when t == 0)."""
    vlo, vhi, rlo, rhi = pcf_ranges(Vi, Ri, n_cell, v_lim, r_lim)
    t = float(mread(cfarFlag, vlo, vhi, rlo, rhi).sum())                              # :259
    if not t > 0:
        return t, [], []
    local_max = np.nanmax(mread(MTD_data, vlo, vhi, rlo, rhi))                        # :261 (max skips NaN)
    r_ind, v_ind = np.nonzero((MTD_data == local_max).T)                              # :262, column-major
    return t, [int(v) + 1 for v in v_ind], [int(r) + 1 for r in r_ind]


def pof_of(Vi, Ri, v_ind, r_ind):
    """:264-271 for scalar v_ind, r_ind."""
    dv = abs(Vi - v_ind)
    dr = abs(Ri - r_ind)
    l = float(dv) ** 2 + float(dr) ** 2                                               # noqa: E741
    l_base = DV_BASE ** 2 + DR_BASE ** 2
    if l < l_base:
        return 1 - l / l_base
    return math.exp(1 - l / l_base) - 1


def fun_PCF(cfarFlag_all, R, V, r_axis, v_axis, frameRInds, MTD_data_all, n_cell=N_CELL, v_lim=V_LIM, r_lim=R_LIM):
    pof_list = []
    for i, R_True, V_True, Ri, Vi in _frames(cfarFlag_all, R, V, r_axis, v_axis, frameRInds):
        MTD_data = np.asarray(MTD_data_all[i - 1])
        cfarFlag = np.asarray(cfarFlag_all[i - 1], np.float64)
        if valid_truth(R_True, V_True):
            t, v_ind, r_ind = pcf_frame(cfarFlag, MTD_data, Vi, Ri, n_cell, v_lim, r_lim)
            if t > 0:
                if len(v_ind) != 1:
                    raise ValueError("dv^2: dv has %d elements (frame %d)" % (len(v_ind), i))
                pof_list.append(pof_of(Vi, Ri, v_ind[0], r_ind[0]))
    return _div(sum(pof_list), len(pof_list))                                         # :278


# ---------------------------------------------------------------------- the device record
def record(cfarFlag, MTD_data, v_idx, r_idx, valid, hv=HV, hr=HR, n_cell=N_CELL, v_lim=V_LIM, r_lim=R_LIM):
    """The 8 ints of rsp_score_dev for one CPI (0-based truth bins), from the pieces above."""
    fl = np.asarray(cfarFlag)
    m, n = fl.shape
    rec = [int(fl.astype(np.int64).sum()), 0, 0, 0, 0, 0, 0, 0]
    if not valid:
        return rec
    Vi, Ri = int(v_idx) + 1, int(r_idx) + 1
    vlo, vhi, rlo, rhi = Vi - hv, Vi + hv, Ri - hr, Ri + hr
    low = vlo < 1 or rlo < 1
    high = vhi > m or rhi > n
    rec[2] = (1 if low else 0) | (2 if high else 0)
    try:
        rec[1] = int(mread(fl, vlo, vhi, rlo, rhi).astype(np.int64).sum())
        assert rec[2] == 0
    except IndexError:
        assert rec[2] != 0
        a, b, c, d = max(vlo, 1), min(vhi, m), max(rlo, 1), min(rhi, n)
        rec[1] = int(fl[a - 1:max(b, a - 1), c - 1:max(d, c - 1)].astype(np.int64).sum())
    try:
        if MTD_data is None:
            t = float(mread(fl, *pcf_ranges(Vi, Ri, n_cell, v_lim, r_lim)).sum())
            v_ind, r_ind = [], []
        else:
            t, v_ind, r_ind = pcf_frame(fl.astype(np.float64), np.asarray(MTD_data), Vi, Ri, n_cell, v_lim, r_lim)
        rec[3] = int(t)
        if v_ind:
            rec[5] = len(v_ind)
            rec[6], rec[7] = v_ind[0] - 1, r_ind[0] - 1
    except IndexError:
        rec[4] = 1
    return rec


def records(flags, rdms, truth_idx, **kw):
    """int32 [batch][8] for a batch; rdms may be None."""
    return np.array([record(flags[b], None if rdms is None else rdms[b], int(t[0]), int(t[1]), int(t[2]), **kw)
                     for b, t in enumerate(np.asarray(truth_idx))], np.int32).reshape(-1, 8)
