"""Detection scoring (main_cfar.m:163-279), CPU side: hand-computed known answers for the
restatement tests/score_ref.py, and rsp_score_summary (host-only C) on records made by the
restatement.  The reference ships no outputs of these functions (they are never called), so
what is pinned is the .m text itself, case by case.
"""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import score_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 40 x 60 frame; axes such that bin k (1-based) is r = 300 + 6 (k-1), v = -19.5 + (k-1)
R_AXIS = 300.0 + 6.0 * np.arange(60)
V_AXIS = -19.5 + np.arange(40)
FLAGS_1B = [(10, 20), (12, 25), (30, 50), (1, 1), (40, 60)]     # (row, column), 1-based


def frame(cells=FLAGS_1B, shape=(40, 60)):
    f = np.zeros(shape, np.uint8)
    for v, r in cells:
        f[v - 1, r - 1] = 1
    return f


def r_of(k):
    return 300.0 + 6.0 * (k - 1)


def v_of(k):
    return -19.5 + (k - 1)


def test_nearest_index_first_of_ties():
    assert sr.nearest_index([0.0, 6.0, 12.0], 3.0) == 1      # tie between bins 1 and 2: the first
    assert sr.nearest_index([0.0, 6.0, 12.0], 9.1) == 3
    assert sr.nearest_index(R_AXIS, r_of(20)) == 20 and sr.nearest_index(V_AXIS, v_of(10)) == 10


def test_validity_gate():
    assert sr.valid_truth(500, -10.5)
    assert not sr.valid_truth(400, -10.5) and not sr.valid_truth(2000, 10)
    assert not sr.valid_truth(500, 3) and not sr.valid_truth(500, -20) and not sr.valid_truth(500, 1.5)


def test_frame_fa_known_answers():
    f = frame()
    # valid, box rows 7..13 x columns 13..27 removes (10,20) and (12,25): 3 of 5 flags are left
    assert sr.fun_frame_fa(f, 500, -10.5, 20, 10) == 3 / 2400
    # not valid: every flag counts
    assert sr.fun_frame_fa(f, 500, 1.5, 20, 10) == 5 / 2400
    # box rows 36..42 x columns 51..65 leaves the matrix on the high side: the copy grows, (40,60) goes
    assert sr.fun_frame_fa(f, 500, 10, 58, 39) == 4 / 2400
    # box rows -1..5: an assignment index below 1 stops MATLAB
    with pytest.raises(IndexError):
        sr.fun_frame_fa(f, 500, 10, 20, 2)
    with pytest.raises(IndexError):
        sr.fun_frame_fa(f, 500, 10, 5, 10)


def test_drate_known_answers():
    fl = np.stack([frame(), frame(), frame()])
    # truths: on the target at (10, 20); valid but on empty cells (25, 35); not valid
    R = [r_of(20), r_of(35), r_of(20)]
    V = [v_of(10), v_of(25), 1.5]
    assert sr.fun_drate(fl, R, V, R_AXIS, V_AXIS, [1, 2, 3]) == 1 / 2
    assert sr.fun_drate(fl[:1], R, V, R_AXIS, V_AXIS, [1]) == 1.0
    assert sr.fun_drate(fl[:1], R, V, R_AXIS, V_AXIS, [2]) == 0.0
    assert math.isnan(sr.fun_drate(fl[:1], R, V, R_AXIS, V_AXIS, [3]))            # 0/0
    # frameRInds index R and V, not the frames
    assert sr.fun_drate(fl[:2], R, V, R_AXIS, V_AXIS, [2, 2]) == 0.0
    # a read outside the matrix stops on either side
    with pytest.raises(IndexError):
        sr.fun_drate(fl[:1], [r_of(58)], [v_of(37)], R_AXIS, V_AXIS, [1])
    with pytest.raises(IndexError):
        sr.fun_drate(fl[:1], [r_of(20)], [v_of(2)], R_AXIS, V_AXIS, [1])


def test_accuracy_quirk():
    empty = np.zeros((40, 60), np.uint8)
    fl = np.stack([frame(), frame(), frame(), empty])
    R = [r_of(20), r_of(35), r_of(20), r_of(20)]
    V = [v_of(10), v_of(25), 1.5, 1.5]
    # frame 1 detects; frame 2 misses; frame 3 is not valid and holds flags -> counts (:224-227);
    # frame 4 is not valid and holds none -> does not
    assert sr.fun_accuracy(fl, R, V, R_AXIS, V_AXIS, [1, 2, 3, 4]) == 2 / 4
    assert sr.fun_accuracy(fl[2:3], R, V, R_AXIS, V_AXIS, [3]) == 1.0
    assert sr.fun_accuracy(fl[3:4], R, V, R_AXIS, V_AXIS, [4]) == 0.0


# fun_PCF needs 41 rows and columns to reach its last three branches: 60 x 80, limits 60 / 80
PV, PR = 60, 80
PCF_KW = dict(n_cell=20, v_lim=PV, r_lim=PR)


@pytest.mark.parametrize("Vi,Ri,want", [
    (5, 40, (1, 25, 20, 60)),        # rows below 1
    (50, 40, (30, 60, 20, 60)),      # rows above v_lim
    (30, 10, (10, 50, 1, 30)),       # columns below 1
    (30, 70, (10, 50, 50, 80)),      # columns above r_lim
    (30, 40, (10, 50, 20, 60)),      # interior
    (5, 10, (1, 25, -10, 30)),       # rows AND columns low: only the first branch clips
    (50, 70, (30, 60, 50, 90)),      # rows AND columns high: the columns stay unclipped
])
def test_pcf_branches(Vi, Ri, want):
    assert sr.pcf_ranges(Vi, Ri, **PCF_KW) == want
    fl = np.zeros((PV, PR), np.uint8)
    mtd = np.zeros((PV, PR), np.float32)
    vlo, vhi, rlo, rhi = want
    if rlo < 1 or rhi > PR:
        with pytest.raises(IndexError):
            sr.pcf_frame(fl, mtd, Vi, Ri, **PCF_KW)
        return
    # a flag on each corner of the clipped box counts; one just outside does not
    for v, r in ((vlo, rlo), (vhi, rhi)):
        fl[v - 1, r - 1] = 1
    if vhi < PV:
        fl[vhi, rlo - 1] = 1
    if rlo > 1:
        fl[vlo - 1, rlo - 2] = 1
    mtd[vlo - 1, rhi - 1] = 7.0
    t, v_ind, r_ind = sr.pcf_frame(fl, mtd, Vi, Ri, **PCF_KW)
    assert t == 2 and v_ind == [vlo] and r_ind == [rhi]


def test_pcf_reference_limits():
    # the literal 155 / 288 of :250-255 on a 155 x 288 matrix
    assert sr.pcf_ranges(140, 100) == (120, 155, 80, 120)
    assert sr.pcf_ranges(100, 280) == (80, 120, 260, 288)
    # on a smaller matrix the hard-coded limits do not protect the read
    with pytest.raises(IndexError):
        sr.pcf_frame(np.zeros((PV, PR)), np.zeros((PV, PR)), 50, 40)


def test_pcf_pof_both_sides_and_repeated_maximum():
    l_base = (1 / 0.2719) ** 2 + 25.0
    fl = np.zeros((1, PV, PR), np.uint8)
    fl[0, 29, 39] = 1
    R, V = [r_of(40)], [v_of(30)]
    r_axis, v_axis = 300.0 + 6.0 * np.arange(PR), -19.5 + np.arange(PV)
    mtd = np.ones((1, PV, PR), np.float32)
    mtd[0, 30, 41] = 9.0       # (31, 42): dv = 1, dr = 2, l = 5 < l_base
    got = sr.fun_PCF(fl, R, V, r_axis, v_axis, [1], mtd, **PCF_KW)
    assert got == 1 - 5 / l_base
    mtd[0, 39, 49] = 11.0      # (40, 50): dv = dr = 10, l = 200 >= l_base
    got = sr.fun_PCF(fl, R, V, r_axis, v_axis, [1], mtd, **PCF_KW)
    assert got == math.exp(1 - 200 / l_base) - 1
    assert -1 < got < 0
    # the same value once more, far outside the box: find() searches the whole matrix
    mtd[0, 0, 79] = 11.0
    with pytest.raises(ValueError):
        sr.fun_PCF(fl, R, V, r_axis, v_axis, [1], mtd, **PCF_KW)
    # no flag in the box: the frame does not score, and the mean of none is NaN
    assert math.isnan(sr.fun_PCF(np.zeros_like(fl), R, V, r_axis, v_axis, [1], mtd, **PCF_KW))
    # two frames: the mean
    fl2 = np.concatenate([fl, fl])
    mtd2 = np.ones((2, PV, PR), np.float32)
    mtd2[0, 30, 41] = 9.0
    mtd2[1, 39, 49] = 9.0
    got = sr.fun_PCF(fl2, R, V, r_axis, v_axis, [1, 1], mtd2, **PCF_KW)
    assert got == ((1 - 5 / l_base) + (math.exp(1 - 200 / l_base) - 1)) / 2


def test_record_fields():
    f = frame()
    assert sr.record(f, None, 9, 19, 0) == [5, 0, 0, 0, 0, 0, 0, 0]
    # v_lim 155 > 40 rows: the PCF box (rows 1..30 by the first branch) fits, columns 0..40 do not
    assert sr.record(f, None, 9, 19, 1) == [5, 2, 0, 0, 1, 0, 0, 0]
    mtd = np.zeros((40, 60), np.float32)
    mtd[11, 24] = 3.0
    mtd[2, 50] = 3.0
    # columns 5..45: rows 1..30 x columns 5..45 hold (10,20), (12,25); the maximum 3.0 twice,
    # first in find() order at column 25 (0-based 24)
    assert sr.record(f, mtd, 9, 24, 1) == [5, 2, 0, 2, 0, 2, 11, 24]
    assert sr.record(f, mtd, 38, 57, 1)[1:3] == [1, 2]       # high side: clipped count, bit 1
    assert sr.record(f, mtd, 1, 4, 1)[1:3] == [1, 1]         # low side: (1,1) in the clipped box, bit 0


# ------------------------------------------------------------------ rsp_score_summary
def _lib():
    from rsp import _capi
    return _capi, _capi.load_library()


def _summary(rec, truth, V, R, **kw):
    from rsp import score
    return score.summary(rec, truth, V, R, score.score_params(**kw))


def _batch(seed, n, clean):
    """n frames of PV x PR with a target (flag blob + RDM peak) and a truth each."""
    rng = np.random.default_rng(seed)
    r_axis, v_axis = 300.0 + 6.0 * np.arange(PR), -19.5 + np.arange(PV)
    fl = (rng.random((n, PV, PR)) < 0.002).astype(np.uint8)
    mtd = rng.random((n, PV, PR)).astype(np.float32)
    R, V = np.empty(n), np.empty(n)
    for i in range(n):
        lo_v, hi_v = (4, 57) if clean else (1, PV)
        lo_r, hi_r = (24, 56) if clean else (18, PR)
        vi, ri = int(rng.integers(lo_v, hi_v + 1)), int(rng.integers(lo_r, hi_r + 1))
        V[i], R[i] = v_axis[vi - 1], r_axis[ri - 1]
        if i % 4 == 3:
            V[i] = 1.0 + 0.1 * (i % 7)               # not valid
        if i % 5 == 4:
            fl[i] = 0                                # no flags at all
        elif i % 3 != 2:                             # a detection near the truth, a peak a few cells off
            pv = min(max(vi + int(rng.integers(-4, 5)), 1), PV)
            pr = min(max(ri + int(rng.integers(-6, 7)), 1), PR)
            fl[i, pv - 1, pr - 1] = 1
            mtd[i, pv - 1, pr - 1] = 5.0 + i
            if not clean and i % 8 == 1:
                mtd[i, (pv + 20) % PV, (pr + 30) % PR] = 5.0 + i    # repeated maximum
    return fl, mtd, R, V, r_axis, v_axis


def _truth(R, V, r_axis, v_axis):
    from rsp import score
    t = score.truth_index(r_axis, v_axis, R, V)
    want = np.array([[sr.nearest_index(v_axis, v) - 1, sr.nearest_index(r_axis, r) - 1, int(sr.valid_truth(r, v))]
                     for r, v in zip(R, V)], np.int32)
    np.testing.assert_array_equal(t, want)
    return t


def test_truth_index_ties_and_gate():
    from rsp import score
    t = score.truth_index([0.0, 6.0, 12.0, 600.0], [-10.0, 0.0, 10.0], [3.0, 600.0, 600.0], [5.0, -5.0, 25.0])
    np.testing.assert_array_equal(t, [[1, 0, 0], [0, 3, 1], [2, 3, 0]])     # ties: the first bin


def test_summary_clean_batch_matches_restatement():
    n = 24
    fl, mtd, R, V, r_axis, v_axis = _batch(11, n, clean=True)
    truth = _truth(R, V, r_axis, v_axis)
    rec = sr.records(fl, mtd, truth, **PCF_KW)
    s = _summary(rec, truth, PV, PR, **PCF_KW)
    ids = list(range(1, n + 1))
    for i in range(n):
        assert s["fa"][i] == sr.fun_frame_fa(fl[i], R[i], V[i], truth[i, 1] + 1, truth[i, 0] + 1)
    assert s["drate"] == sr.fun_drate(fl, R, V, r_axis, v_axis, ids)
    assert s["acc"] == sr.fun_accuracy(fl, R, V, r_axis, v_axis, ids)
    want_pof = sr.fun_PCF(fl, R, V, r_axis, v_axis, ids, mtd, **PCF_KW)
    assert abs(s["pof"] - want_pof) <= 1e-14
    assert 0 < s["drate"] < 1 and 0 < s["acc"] < 1 and s["n_scored"] >= 5
    assert s["n_valid"] == int(truth[:, 2].sum())
    assert s["n_index_error"] == dict(fa=0, drate=0, acc=0, pcf=0) and s["n_multi_peak"] == 0


def test_summary_counts_what_the_reference_stops_at():
    n = 48
    fl, mtd, R, V, r_axis, v_axis = _batch(12, n, clean=False)
    truth = _truth(R, V, r_axis, v_axis)
    rec = sr.records(fl, mtd, truth, **PCF_KW)
    s = _summary(rec, truth, PV, PR, **PCF_KW)
    err = dict(fa=0, drate=0, acc=0, pcf=0)
    multi = 0
    ok_d, ok_p, acc_count = [], [], 0.0
    for i in range(n):
        one = (fl[i:i + 1], [R[i]], [V[i]], r_axis, v_axis, [1])
        try:
            assert s["fa"][i] == sr.fun_frame_fa(fl[i], R[i], V[i], truth[i, 1] + 1, truth[i, 0] + 1)
        except IndexError:
            err["fa"] += 1
            assert math.isnan(s["fa"][i])
        try:
            sr.fun_drate(*one)
            ok_d.append(i)
        except IndexError:
            err["drate"] += 1
        try:
            acc_count += sr.fun_accuracy(*one)
        except IndexError:
            err["acc"] += 1
        try:
            sr.fun_PCF(*one, mtd[i:i + 1], **PCF_KW)
            ok_p.append(i)
        except IndexError:
            err["pcf"] += 1
        except ValueError:
            multi += 1
    assert s["n_index_error"] == err and s["n_multi_peak"] == multi
    assert min(err.values()) > 0 and multi > 0 and err["fa"] < err["drate"]
    assert s["drate"] == sr.fun_drate(fl[ok_d], R[ok_d], V[ok_d], r_axis, v_axis, list(range(1, len(ok_d) + 1)))
    assert s["acc"] == acc_count / n
    want_pof = sr.fun_PCF(fl[ok_p], R[ok_p], V[ok_p], r_axis, v_axis, list(range(1, len(ok_p) + 1)), mtd[ok_p], **PCF_KW)
    assert abs(s["pof"] - want_pof) <= 1e-14


def test_summary_nan_cases():
    # no valid truth: drate 0/0, pof mean of none; acc from the any-flag rule
    fl = np.stack([frame(), np.zeros((40, 60), np.uint8)])
    truth = np.array([[9, 19, 0], [9, 19, 0]], np.int32)
    s = _summary(sr.records(fl, None, truth), truth, 40, 60)
    assert math.isnan(s["drate"]) and math.isnan(s["pof"]) and s["acc"] == 0.5
    np.testing.assert_array_equal(s["fa"], [5 / 2400, 0.0])
    assert s["n_valid"] == 0 and s["n_scored"] == 0


def test_score_struct_layouts_match_header():
    _capi, _ = _lib()
    src = ('#include "rsp.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %d\\n",'
           ' sizeof(rsp_score_params), sizeof(rsp_score_result), offsetof(rsp_score_params, ld),'
           ' offsetof(rsp_score_result, n_index_error), offsetof(rsp_score_result, n_multi_peak),'
           ' RSP_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(_capi.rsp_score_params), C.sizeof(_capi.rsp_score_result), _capi.rsp_score_params.ld.offset,
                   _capi.rsp_score_result.n_index_error.offset, _capi.rsp_score_result.n_multi_peak.offset, 5]


def test_score_null_arguments():
    _capi, lib = _lib()
    p = _capi.rsp_score_params()
    out = _capi.rsp_score_result()
    rec = np.zeros((1, 8), np.int32)
    tr = np.zeros((1, 3), np.int32)
    assert lib.rsp_score_dev(None, None, None, 4, 4, 1, C.byref(p), None, None, None) == _capi.RSP_ERR_ARG
    assert b"rsp_score_dev" in lib.rsp_last_error(None)
    ok = (rec.ctypes.data, tr.ctypes.data, 1, 4, 4, C.byref(p), None, C.byref(out))
    assert lib.rsp_score_summary(*ok) == _capi.RSP_OK
    for k in (0, 1, 5, 7):
        bad = list(ok)
        bad[k] = None
        assert lib.rsp_score_summary(*bad) == _capi.RSP_ERR_ARG, k
        assert b"rsp_score_summary" in lib.rsp_last_error(None)
    assert lib.rsp_score_summary(rec.ctypes.data, tr.ctypes.data, -1, 4, 4, C.byref(p), None, C.byref(out)) == _capi.RSP_ERR_ARG
