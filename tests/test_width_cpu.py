"""Doppler line width, CPU side: the restatement tests/width_ref.py against hand-computed cases of
ampConstrWidthEst.m's text, its spline against scipy's not-a-knot CubicSpline, the tie condition
on the GPU tests' own scenes, and the C ABI's declaration, struct layout and refusals
(rsp_spec_width_dev checks everything it can before it looks at the context).
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import width_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _w(y_shifted, a, flag, interp):
    """The width of one column given as the .m sees it after its fftshift."""
    first, last, width, margin = wr.width(np.fft.ifftshift(np.asarray(y_shifted, np.float64)), a, flag, interp)
    return int(first[0]), int(last[0]), float(width[0]), float(margin[0])


# ---------------------------------------------------------------- the .m text by hand
def test_one_two_four_two_one():
    # 20*log10(2/4) = -6.0206 dB: inside at -6.03, outside at -6.0
    assert _w([1, 2, 4, 2, 1], -6.03, 0, 1)[:3] == (1, 3, 2.0)
    assert _w([1, 2, 4, 2, 1], -6.0, 0, 1)[:3] == (2, 2, 0.0)
    # interpTimes = 1 with the flag set is the same samples
    assert _w([1, 2, 4, 2, 1], -6.03, 1, 1)[:3] == (1, 3, 2.0)
    # the margin is the nearest sample's distance from the level over M1
    m = _w([1, 2, 4, 2, 1], -6.03, 0, 1)[3]
    assert abs(m - abs(2.0 - 10 ** (-6.03 / 20) * 4.0) / 4.0) < 1e-15


def test_rotation_odd_and_even():
    # fftshift moves element i to (i + floor(V/2)) mod V
    for V in (4, 5, 8, 9):
        x = np.zeros(V)
        x[0] = 1.0                      # lands on floor(V/2)
        x[1] = 0.6                      # on floor(V/2) + 1
        first, last, width, _ = wr.width(x, -6.0, 0, 1)
        assert (first[0], last[0], width[0]) == (V // 2, V // 2 + 1, 1.0), V
        first, last, _, _ = wr.width(x, -6.0, 0, 1, shift=False)
        assert (first[0], last[0]) == (0, 1)
        np.testing.assert_array_equal(wr.samples(x, 1, False, True)[1][:, 0], np.fft.fftshift(x))


def test_all_zero_column_and_single_sample():
    first, last, width, margin = wr.width(np.zeros((8, 2)), -6.0, 1, 4)
    assert first.tolist() == [-1, -1] and last.tolist() == [-1, -1] and width.tolist() == [0.0, 0.0]
    assert np.isinf(margin).all()
    assert _w([0, 0, 0, 5, 0, 0, 0, 0], -6.0, 0, 1)[:3] == (3, 3, 0.0)
    # on the fine grid the line has a width of its own: a few samples round the knot
    f, l, w, _ = _w([0, 0, 0, 5, 0, 0, 0, 0], -6.0, 1, 8)
    assert f < 24 < l and w == (l - f) / 8.0 and w < 2.0


def test_two_lines_span_the_gap():
    y = np.zeros(32)
    y[5], y[20] = 10.0, 8.0
    assert _w(y, -3.0, 0, 1)[:3] == (5, 20, 15.0)          # 8/10 = -1.94 dB: both inside
    assert _w(y, -1.0, 0, 1)[:3] == (5, 5, 0.0)
    f, l, w, _ = _w(y, -3.0, 1, 4)
    assert f <= 20 and l >= 80 and w == (l - f) / 4.0      # from the first line's skirt to the second's


def test_spline_undershoot_counts_by_modulus():
    """Beside a zeroed band the spline rings below zero; MATLAB's log10 of the negative ratio is
    complex and >= compares its real part, 20*log10|s/M1|: at a level low enough the negative
    lobes are inside the span."""
    y = np.zeros(24)
    y[8] = 100.0
    x, s = wr.samples(np.fft.ifftshift(y), 8, True, True)
    assert s.min() < -1.0                                   # a real undershoot
    neg = np.flatnonzero(s[:, 0] < 0)
    lvl = 20 * np.log10(np.abs(s[neg, 0]).max() / s.max()) - 1.0
    f, l, _, _ = _w(y, lvl, 1, 8)
    inside = [i for i in neg if f <= i <= l and 20 * np.log10(abs(s[i, 0]) / s.max()) >= lvl]
    assert inside                                           # selected although negative
    # the first selected sample is itself an undershoot or lies before one
    assert f <= neg[np.abs(s[neg, 0]).argmax()] <= l
    # the same column with the sign rule (s >= level * M1) would start later or end sooner
    pos = np.flatnonzero(s[:, 0] >= 10 ** (lvl / 20) * s.max())
    assert f < pos[0] or l > pos[-1]


# ---------------------------------------------------------------- the spline against scipy
@pytest.mark.parametrize("V", [4, 5, 33, 2048])
def test_spline_against_scipy(V):
    interpolate = pytest.importorskip("scipy.interpolate")
    y = wr.scene(V, 3, seed=900 + V).astype(np.float64)
    x = wr.colon_unit(V, 8)
    got = wr.spline_eval(y, wr.spline_m(y), x)
    want = interpolate.CubicSpline(np.arange(V), y, axis=0, bc_type="not-a-knot")(x)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(y))
    # through its knots (to rounding: colon's second half counts back from V-1 in steps of 1/8,
    # and the last knot is the last interval at u = 1)
    assert np.max(np.abs(got[::8] - y)) <= 1e-15 * np.max(np.abs(y))
    assert x[0] == 0.0 and x[-1] == V - 1 and len(x) == (V - 1) * 8 + 1


# ---------------------------------------------------------------- ties on the GPU tests' scenes
def _tie_stats(amp, need, interp, shift):
    out = []
    idx = np.flatnonzero(need)
    x, s = wr.samples(amp[:, idx], interp, True, shift)
    for lv in wr.LEVELS:
        margin = wr.select(x, s, lv, interp)[3]
        out.append((int(idx.size), int((margin <= wr.TIE).sum()), float(margin.min())))
    return out


def test_scenes_have_no_tie_columns():
    """By the restatement alone: none of the columns the GPU tests compare is a tie column (the
    nearest sample lies more than 1e-9 of M1 from the level), at every V, interp, level and shift
    they use."""
    tested = ties = 0
    least = np.inf
    for V, R in wr.SHAPES:
        amp = wr.scene(V, R, seed=V)
        for interp in wr.interps_for(V):
            for shift in (0, 1):
                for n, t, m in _tie_stats(amp, np.ones(R, bool), interp, shift):
                    tested, ties, least = tested + n, ties + t, min(least, m)
    w = wr.WIN
    for b in range(w["batch"]):
        amp = wr.scene(w["V"], w["R"], seed=70 + b)
        for n, t, m in _tie_stats(amp, np.ones(w["R"], bool), 4, 1) + _tie_stats(amp, np.ones(w["R"], bool), 3, 0):
            tested, ties, least = tested + n, ties + t, min(least, m)
    d = wr.DMX
    amp = wr.scene(d["V"], d["Rp"], seed=2048574)
    flag = wr.sparse_flags(d["V"], d["Rp"], d["hits"], seed=11)
    for n, t, m in _tie_stats(amp, flag.any(axis=0), 4, 1)[1:2] + _tie_stats(amp, flag.any(axis=0), 8, 1)[1:2]:
        tested, ties, least = tested + n, ties + t, min(least, m)
    assert tested > 2000 and ties == 0, (tested, ties, least)
    assert least > wr.TIE


# ---------------------------------------------------------------- the C boundary
def _lib():
    from rsp import _capi
    return _capi, _capi.load_library()


def test_header_declares_and_library_exports():
    _capi, lib = _lib()
    text = open(os.path.join(ROOT, "include", "rsp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+rsp_spec_width_dev\s*\(", text)
    assert hasattr(lib, "rsp_spec_width_dev") and "rsp_spec_width_dev" in _capi.EXPORTS
    assert re.search(r"#define\s+RSP_WIDTH_MIN_V\s+4\b", text) and _capi.RSP_WIDTH_MIN_V == 4
    assert re.search(r"#define\s+RSP_WIDTH_MAX_V\s+2048\b", text) and _capi.RSP_WIDTH_MAX_V == 2048
    import rsp
    assert rsp.ampConstrWidthEst is rsp.width.ampConstrWidthEst and hasattr(rsp.width.Width, "width_dev")


def test_struct_layout_matches_header():
    _capi, _ = _lib()
    cls = _capi.rsp_width_params
    fields = [n for n, _ in cls._fields_]
    assert fields == ["amp_constr", "interp", "shift", "ld", "cpi_stride"]
    src = ('#include "rsp.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu", sizeof(rsp_width_params));\n'
           + "".join('printf(" %%zu", offsetof(rsp_width_params, %s));\n' % f for f in fields)
           + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]


def test_null_and_malformed_arguments():
    """Everything is refused before the context is looked at: no GPU needed (ctx == NULL; the
    addresses are never touched)."""
    _capi, lib = _lib()
    amp, flag, span, count = 0x10000, 0x20000, 0x30000, 0x40000

    def P(a=-6.0, interp=4, shift=1, ld=0, cs=0):
        p = _capi.rsp_width_params()
        p.amp_constr, p.interp, p.shift, p.ld, p.cpi_stride = a, interp, shift, ld, cs
        return p

    def call(p, amp=amp, flag=flag, span=span, count=count, V=128, R=20, B=3):
        return lib.rsp_spec_width_dev(None, amp, flag, V, R, B, C.byref(p) if p is not None else None, span, count,
                                      None)

    def msg():
        return lib.rsp_last_error(None).decode()

    ARG = _capi.RSP_ERR_ARG
    # a well-formed call gets as far as the null context; d_flag may be NULL
    assert call(P()) == ARG and "null ctx" in msg()
    assert call(P(), flag=None) == ARG and "null ctx" in msg()
    assert call(P(a=-200.0, interp=1, shift=0, ld=20, cs=127 * 20 + 20), V=128) == ARG and "null ctx" in msg()
    assert call(P(a=-1e-9, interp=64), V=4) == ARG and "null ctx" in msg()
    assert call(P(), V=2048, R=1, B=0) == ARG and "null ctx" in msg()
    for kw in (dict(amp=None), dict(span=None), dict(count=None)):
        assert call(P(), **kw) == ARG and "null argument" in msg(), kw
    assert call(None) == ARG and "null argument" in msg()
    # the level
    for a in (0.0, 3.0, -200.5, float("nan"), float("-inf")):
        assert call(P(a=a)) == ARG and "amp_constr" in msg(), a
    # interp, shift
    for i in (0, 65, -1):
        assert call(P(interp=i)) == ARG and "interp" in msg(), i
    assert call(P(shift=2)) == ARG and "shift" in msg()
    # V
    for V in (3, 2049, 0, -4):
        assert call(P(), V=V) == ARG and "V =" in msg(), V
    # shape and pitches
    assert call(P(), R=0) == ARG and "bad shape" in msg()
    assert call(P(), B=-1) == ARG and "bad shape" in msg()
    assert call(P(ld=19)) == ARG and "row pitch" in msg()
    assert call(P(ld=20)) == ARG and "null ctx" in msg()
    assert call(P(ld=32, cs=127 * 32 + 19)) == ARG and "CPI stride" in msg()
    assert call(P(ld=32, cs=127 * 32 + 20)) == ARG and "null ctx" in msg()
    assert call(P(ld=-1)) == ARG and "negative" in msg()
    assert call(P(cs=-1)) == ARG and "negative" in msg()
