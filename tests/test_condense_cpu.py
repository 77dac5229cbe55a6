"""Plot condensation, CPU side: the restatement tests/condense_ref.py pinned against
scipy.ndimage.label and hand-worked cases, and the C ABI's declaration, struct layout and
refusals (rsp_condense_dev checks everything it can before it looks at the context).
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import condense_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_plane(V, R, density, seed):
    rng = np.random.default_rng(seed)
    flag = (rng.random((V, R)) < density).astype(np.uint8)
    amp = rng.random((V, R)).astype(np.float32) + 0.5
    return amp, flag


@pytest.mark.parametrize("V,R,density", [(33, 17, 0.30), (96, 130, 0.06), (96, 130, 0.45), (64, 40, 0.01)])
@pytest.mark.parametrize("gap", [(1, 1), (2, 1)])
def test_components_match_scipy_label(V, R, density, gap):
    """gap (1, 1) is label's 3 x 3 structure.  gap (2, 1) is a 5 x 3 neighbourhood, and label takes
    3 x 3 structures only ("structure dimensions must be equal to 3"), so it is given the same
    relation in that form: every hit also occupies the cell below it (in a plane one row taller).
    Cells (v+a, r), (v'+b, r'), a, b in {0, 1}, touch under the 3 x 3 structure for some a, b
    exactly when |v - v'| <= 2 and |r - r'| <= 1; each hit is then labelled at its own cell."""
    from scipy import ndimage
    amp, flag = _random_plane(V, R, density, seed=V * 1000 + R)
    if gap == (1, 1):
        lab, n = ndimage.label(flag, structure=np.ones((3, 3)))
    else:
        tall = np.zeros((V + 1, R), np.uint8)
        tall[:V] = flag
        tall[1:] |= flag
        lab, n = ndimage.label(tall, structure=np.ones((3, 3)))
        lab = lab[:V] * (flag != 0)
    peak, plots, (n_plots, n_hits) = condense_ref.condense(amp, flag, gap=gap, wrap_v=False)
    assert n_hits == int(flag.sum())
    assert n_plots == n == len(plots) == int(peak.sum())
    sizes = np.sort(np.bincount(lab.ravel())[1:])
    np.testing.assert_array_equal(np.sort(plots[:, 2]), sizes)
    # every component holds exactly one peak, and it is the component's first maximum
    for k in range(1, n + 1):
        m = lab == k
        assert int(peak[m].sum()) == 1
        v, r = np.nonzero(peak & m)
        cand = np.argwhere(m & (amp == amp[m].max()))
        first = min((int(c[1]) * V + int(c[0]), int(c[0]), int(c[1])) for c in cand)
        assert (int(v[0]), int(r[0])) == first[1:]
    # plots are in peak find() order and their boxes are those of the labels
    keys = plots[:, 1].astype(np.int64) * V + plots[:, 0]
    assert np.all(np.diff(keys) > 0)
    for p in plots:
        m = lab == lab[p[0], p[1]]
        vv, rr = np.nonzero(m)
        assert tuple(p[2:]) == (m.sum(), vv.min(), vv.max(), rr.min(), rr.max(), 0)


def _one(flag, amp=None, **kw):
    flag = np.asarray(flag, dtype=np.uint8)
    if amp is None:
        amp = np.ones(flag.shape, dtype=np.float32)
    return condense_ref.condense(amp, flag, **kw)


def test_plateau_takes_first_in_find_order():
    flag = np.zeros((6, 5), np.uint8)
    amp = np.zeros((6, 5), np.float32)
    # an L of three equal cells: (3, 1), (2, 2), (3, 2): find() order is column 1 first
    for v, r in ((3, 1), (2, 2), (3, 2)):
        flag[v, r] = 1
        amp[v, r] = 7.0
    peak, plots, n = _one(flag, amp)
    assert n == (1, 3) and plots.tolist() == [[3, 1, 3, 2, 3, 1, 2, 0]]
    assert peak[3, 1] == 1 and peak.sum() == 1
    # within one column the smaller row wins
    flag[:] = 0
    flag[2:5, 3] = 1
    amp[2:5, 3] = 2.0
    peak, plots, n = _one(flag, amp)
    assert plots.tolist() == [[2, 3, 3, 2, 4, 3, 3, 0]]
    # a strictly larger later cell wins over the earlier ones
    amp[4, 3] = 2.5
    assert _one(flag, amp)[1].tolist() == [[4, 3, 3, 2, 4, 3, 3, 0]]


@pytest.mark.parametrize("gap", [(1, 1), (2, 1), (0, 3), (4, 4)])
def test_gap_and_gap_plus_one(gap):
    gv, gr = gap
    V, R = 24, 24
    for axis in (0, 1):
        g = gap[axis]
        for d, want in ((g, 1), (g + 1, 2)):
            if d == 0:
                continue
            flag = np.zeros((V, R), np.uint8)
            flag[5, 6] = 1
            flag[5 + (d if axis == 0 else 0), 6 + (d if axis == 1 else 0)] = 1
            assert _one(flag, gap=gap)[2] == (want, 2), (gap, axis, d)
    # both offsets at their gaps at once still join; one past in either does not
    flag = np.zeros((V, R), np.uint8)
    flag[5, 6] = flag[5 + gv, 6 + gr] = 1
    assert _one(flag, gap=gap)[2][0] == (1 if (gv, gr) != (0, 0) else 2)


def test_seam_joins_only_with_wrap():
    V, R = 16, 9
    flag = np.zeros((V, R), np.uint8)
    flag[0, 4] = flag[V - 1, 4] = 1
    assert _one(flag, wrap_v=False)[2] == (2, 2)
    peak, plots, n = _one(flag, wrap_v=True)
    assert n == (1, 2) and plots.tolist() == [[0, 4, 2, 0, V - 1, 4, 4, 0]]     # v_min, v_max are plain
    # a diagonal across the seam
    flag[:] = 0
    flag[V - 2, 2] = flag[V - 1, 3] = flag[0, 4] = flag[1, 5] = 1
    assert _one(flag, wrap_v=False)[2] == (2, 4)
    peak, plots, n = _one(flag, wrap_v=True)
    assert n == (1, 4) and plots.tolist() == [[V - 2, 2, 4, 0, V - 1, 2, 5, 0]]
    # gap_v = 2 reaches from row V-1 to row 1, not to row 2
    flag[:] = 0
    flag[V - 1, 0] = flag[1, 0] = 1
    assert _one(flag, gap=(2, 0), wrap_v=True)[2] == (1, 2)
    flag[:] = 0
    flag[V - 1, 0] = flag[2, 0] = 1
    assert _one(flag, gap=(2, 0), wrap_v=True)[2] == (2, 2)


def test_gap_zero_empty_and_full():
    amp, flag = _random_plane(12, 10, 0.5, seed=3)
    peak, plots, n = _one(flag, amp, gap=(0, 0))
    assert n == (int(flag.sum()), int(flag.sum()))
    np.testing.assert_array_equal(peak, flag)
    v, r = condense_ref.hits(flag)
    np.testing.assert_array_equal(plots[:, 0], v)
    np.testing.assert_array_equal(plots[:, 1], r)
    assert np.all(plots[:, 2] == 1)
    peak, plots, n = _one(np.zeros((7, 5)))
    assert n == (0, 0) and peak.sum() == 0 and plots.shape == (0, 8)
    amp = np.arange(35, dtype=np.float32).reshape(7, 5)
    peak, plots, n = _one(np.ones((7, 5)), amp)
    assert n == (1, 35) and plots.tolist() == [[6, 4, 35, 0, 6, 0, 4, 0]]


# ---------------------------------------------------------------- the C boundary
def _lib():
    from rsp import _capi
    return _capi, _capi.load_library()


def test_header_declares_and_library_exports():
    _capi, lib = _lib()
    text = open(os.path.join(ROOT, "include", "rsp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+rsp_condense_dev\s*\(", text)
    assert hasattr(lib, "rsp_condense_dev") and "rsp_condense_dev" in _capi.EXPORTS


def test_struct_layout_matches_header():
    _capi, _ = _lib()
    fields = ("gap_v", "gap_r", "wrap_v", "reserved", "ld", "cpi_stride")
    src = ('#include "rsp.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu", sizeof(rsp_condense_params));\n'
           + "".join('printf(" %%zu", offsetof(rsp_condense_params, %s));\n' % f for f in fields)
           + 'printf(" %d\\n", RSP_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    want = ([C.sizeof(_capi.rsp_condense_params)] + [getattr(_capi.rsp_condense_params, f).offset for f in fields] + [5])
    assert got == want


def test_null_and_malformed_arguments():
    """Everything is refused before the context is looked at: no GPU needed (ctx == NULL; the
    addresses are never touched)."""
    _capi, lib = _lib()
    amp, flag, peak, plots, count = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000

    def params(gap=(1, 1), wrap_v=0, ld=0, cs=0, reserved=0):
        p = _capi.rsp_condense_params()
        p.gap_v, p.gap_r, p.wrap_v, p.reserved, p.ld, p.cpi_stride = gap[0], gap[1], wrap_v, reserved, ld, cs
        return p

    def call(p, amp=amp, flag=flag, peak=peak, plots=plots, count=count, V=32, R=20, B=3, max_plots=16):
        return lib.rsp_condense_dev(None, amp, flag, V, R, B, C.byref(p) if p is not None else None, peak,
                                    max_plots, plots, count, None)

    def msg():
        return lib.rsp_last_error(None).decode()

    ARG, UNS = _capi.RSP_ERR_ARG, _capi.RSP_ERR_UNSUPPORTED
    # a well-formed call gets as far as the null context; d_plots may be NULL
    assert call(params()) == ARG and "null ctx" in msg()
    assert call(params(), plots=None) == ARG and "null ctx" in msg()
    assert call(params(gap=(4, 4), wrap_v=1, ld=24, cs=32 * 24 + 5)) == ARG and "null ctx" in msg()
    for kw in (dict(amp=None), dict(flag=None), dict(peak=None), dict(count=None)):
        assert call(params(), **kw) == ARG and "null argument" in msg(), kw
    assert call(None) == ARG and "null argument" in msg()
    for gap in ((-1, 1), (5, 1), (1, -1), (1, 5)):
        assert call(params(gap=gap)) == ARG and "outside 0..4" in msg(), gap
    assert call(params(wrap_v=2)) == ARG and "wrap_v" in msg()
    assert call(params(reserved=1)) == ARG and "reserved" in msg()
    # wrap_v needs V > 2*gap_v
    assert call(params(gap=(2, 1), wrap_v=1), V=4) == ARG and "2*gap_v" in msg()
    assert call(params(gap=(2, 1), wrap_v=1), V=5) == ARG and "null ctx" in msg()
    assert call(params(gap=(2, 1), wrap_v=0), V=4) == ARG and "null ctx" in msg()
    assert call(params(gap=(0, 1), wrap_v=1), V=1) == ARG and "null ctx" in msg()
    # pitches
    assert call(params(ld=19)) == ARG and "row pitch" in msg()
    assert call(params(ld=24, cs=31 * 24 + 19)) == ARG and "row pitch" in msg()
    assert call(params(), peak=flag) == ARG and "d_peak == d_flag" in msg()
    assert call(params(), V=0) == ARG and "bad shape" in msg()
    assert call(params(), B=-1) == ARG and "bad shape" in msg()
    assert call(params(), max_plots=-1) == ARG and "bad shape" in msg()
    # the cell index is int32
    assert call(params(), V=1 << 16, R=1 << 15) == UNS and "int32" in msg()
    assert call(params(), V=(1 << 16) - 1, R=1 << 15) == ARG and "null ctx" in msg()
    assert call(params(), V=1 << 40, R=1 << 40) == UNS
