"""Target injection at a set SCR (fun_SCR.m / fun_add_clutter.m), CPU side: the C ABI's
declarations, struct layout and refusals, the host export of the gain function the kernel calls
(rsp_scr_gain) against the fp64 restatement tests/scr_ref.py, and target_plan's geometry.
"""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import scr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from rsp import _capi
    return _capi, _capi.load_library()


def test_header_declares_and_library_exports():
    _capi, lib = _lib()
    text = open(os.path.join(ROOT, "include", "rsp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("rsp_scr_dev", "rsp_inject_dev", "rsp_scr_gain"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in _capi.EXPORTS
    assert "RSP_SCR_ABS2 = 0" in text and "RSP_SCR_AS_WRITTEN = 1" in text
    assert (_capi.RSP_SCR_ABS2, _capi.RSP_SCR_AS_WRITTEN) == (0, 1)


def test_scr_struct_layout_matches_header():
    _capi, _ = _lib()
    fields = ("nseg", "power", "add_clutter", "reserved", "seg_start", "seg_len", "seg_db", "clutter_ld", "clutter_batch")
    src = ('#include "rsp.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu", sizeof(rsp_scr_params));\n'
           + "".join('printf(" %%zu", offsetof(rsp_scr_params, %s));\n' % f for f in fields)
           + 'printf(" %d\\n", RSP_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    want = [C.sizeof(_capi.rsp_scr_params)] + [getattr(_capi.rsp_scr_params, f).offset for f in fields] + [5]
    assert got == want


def _params(segments=((0, 8), (8, 8)), **kw):
    from rsp import inject
    return inject.scr_params(segments, **kw)


def test_null_and_malformed_arguments():
    """Everything is refused before the context is looked at: no GPU needed (ctx == NULL; the
    pointers are never dereferenced)."""
    _capi, lib = _lib()
    P, R, B = 4, 16, 3
    simu, clut, out, scr = 0x10000, 0x20000, 0x30000, 0x40000      # device addresses that are never touched
    n = B * P * R * 8

    def scr_dev(p, simu=simu, clut=clut, out=out, scr=scr, P=P, R=R, B=B):
        return lib.rsp_scr_dev(None, simu, clut, out, P, R, B, scr, C.byref(p) if p is not None else None, None)

    def msg():
        return lib.rsp_last_error(None).decode()

    # a well-formed call gets as far as the null context
    assert scr_dev(_params()) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    for kw in (dict(simu=None), dict(clut=None), dict(out=None), dict(scr=None)):
        assert scr_dev(_params(), **kw) == _capi.RSP_ERR_ARG and "null argument" in msg(), kw
    assert scr_dev(None) == _capi.RSP_ERR_ARG and "null argument" in msg()
    assert scr_dev(_params(), P=0) == _capi.RSP_ERR_ARG and "bad shape" in msg()
    assert scr_dev(_params(), B=-1) == _capi.RSP_ERR_ARG and "bad shape" in msg()
    # segments: overlapping, out of range, empty, too many
    assert scr_dev(_params(((0, 9), (8, 8)))) == _capi.RSP_ERR_ARG and "overlap" in msg()
    assert scr_dev(_params(((8, 8), (0, 9)))) == _capi.RSP_ERR_ARG and "overlap" in msg()
    assert scr_dev(_params(((0, 8), (8, 9)))) == _capi.RSP_ERR_ARG and "not inside" in msg()
    assert scr_dev(_params(((-1, 4),))) == _capi.RSP_ERR_ARG and "not inside" in msg()
    assert scr_dev(_params(((3, 0),))) == _capi.RSP_ERR_ARG and "not inside" in msg()
    p = _params()
    p.nseg = _capi.RSP_MAX_SEG + 1
    assert scr_dev(p) == _capi.RSP_ERR_ARG and "nseg" in msg()
    p.nseg = -1
    assert scr_dev(p) == _capi.RSP_ERR_ARG and "nseg" in msg()
    p = _params()
    p.power = 2
    assert scr_dev(p) == _capi.RSP_ERR_ARG and "power" in msg()
    # clutter geometry
    assert scr_dev(_params(clutter_batch=B + 1)) == _capi.RSP_ERR_ARG and "clutter_batch" in msg()
    assert scr_dev(_params(clutter_batch=-1)) == _capi.RSP_ERR_ARG and "clutter_batch" in msg()
    assert scr_dev(_params(clutter_ld=R - 1)) == _capi.RSP_ERR_ARG and "clutter_ld" in msg()
    # aliasing: out == simu is fine, out == clutter only with the full geometry, partial overlaps never
    assert scr_dev(_params(), out=simu) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    assert scr_dev(_params(), out=clut) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    assert scr_dev(_params(clutter_batch=B, clutter_ld=R), out=clut) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    assert scr_dev(_params(clutter_batch=2), out=clut) == _capi.RSP_ERR_ARG and "d_out == d_clutter" in msg()
    assert scr_dev(_params(clutter_ld=R + 2), out=clut) == _capi.RSP_ERR_ARG and "d_out == d_clutter" in msg()
    assert scr_dev(_params(), out=simu + 8) == _capi.RSP_ERR_ARG and "overlaps d_simu" in msg()
    assert scr_dev(_params(), out=clut + n - 8) == _capi.RSP_ERR_ARG and "overlaps d_clutter" in msg()
    assert scr_dev(_params(), out=out + 4) == _capi.RSP_ERR_ARG and "aligned" in msg()

    # the point-target form shares the checks and adds its own
    off = (C.c_int64 * 3)(0, 4, 10)
    wf, delay, dphi = 0x50000, 0x60000, 0x70000

    def inject_dev(p, off=off, wf=wf, delay=delay, dphi=dphi, out=out):
        return lib.rsp_inject_dev(None, clut, out, P, R, B, wf, off, delay, dphi, scr, C.byref(p), None)

    assert inject_dev(_params()) == _capi.RSP_ERR_ARG and "null ctx" in msg()
    for kw in (dict(off=None), dict(wf=None), dict(delay=None), dict(dphi=None)):
        assert inject_dev(_params(), **kw) == _capi.RSP_ERR_ARG and "null argument" in msg(), kw
    assert inject_dev(_params(), off=(C.c_int64 * 3)(0, 4, 3)) == _capi.RSP_ERR_ARG and "wf_off" in msg()
    assert inject_dev(_params(((0, 9), (8, 8)))) == _capi.RSP_ERR_ARG and "overlap" in msg()
    assert inject_dev(_params(clutter_batch=2), out=clut) == _capi.RSP_ERR_ARG and "d_out == d_clutter" in msg()

    g = (C.c_double * 2)()
    one = (C.c_double * 2)(1.0, 0.0)
    assert lib.rsp_scr_gain(0, None, one, 4, 0.0, g) == _capi.RSP_ERR_ARG and "rsp_scr_gain" in msg()
    assert lib.rsp_scr_gain(0, one, one, 0, 0.0, g) == _capi.RSP_ERR_ARG
    assert lib.rsp_scr_gain(2, one, one, 4, 0.0, g) == _capi.RSP_ERR_ARG
    assert lib.rsp_scr_gain(0, one, one, 4, 0.0, None) == _capi.RSP_ERR_ARG


def _c_gain(power, ss, sc, n, db):
    _capi, lib = _lib()
    a = (C.c_double * 2)(ss.real, ss.imag)
    b = (C.c_double * 2)(sc.real, sc.imag)
    g = (C.c_double * 2)()
    assert lib.rsp_scr_gain(power, a, b, n, db, g) == _capi.RSP_OK
    return complex(g[0], g[1])


def _close(got, want, rel=1e-14):
    assert abs(got - want) <= rel * abs(want), (got, want)


@pytest.mark.parametrize("power", [scr_ref.ABS2, scr_ref.AS_WRITTEN])
def test_gain_matches_restatement(power):
    rng = np.random.default_rng(7)
    for n in (1, 82, 242, 707, 4096):
        for db in (-30.0, -5.0, 0.0, 3.3, 10.0, 20.0):
            x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
            c = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 10.0 ** rng.uniform(-2, 2)
            ss, sc = scr_ref.power_sum(x, power), scr_ref.power_sum(c, power)
            want = scr_ref.gain_from_sums(power, ss, sc, n, db)
            got = _c_gain(power, ss, sc, n, db)
            _close(got, want)
            # the principal root: the right half plane
            assert got.real >= 0
            if power == scr_ref.ABS2:
                assert got.imag == 0.0
                # achieved SCR: |gain|^2 * P_s / P_echo
                assert abs(got.real ** 2 * (ss.real / n) / (sc.real / n) / 10.0 ** (db / 10.0) - 1) < 1e-12


def test_gain_edge_cases():
    n = 64
    # a negative real g as written: target squares sum to a negative real, clutter's to a positive one
    want = scr_ref.gain_from_sums(scr_ref.AS_WRITTEN, -32.0 + 0j, 128.0 + 0j, n, 0.0)
    got = _c_gain(scr_ref.AS_WRITTEN, -32.0 + 0j, 128.0 + 0j, n, 0.0)
    assert want.real == 0.0 and abs(want.imag - 2.0) < 1e-14       # +j sqrt|g|, g = -4 (up to eps)
    assert got.real == 0.0 and got.imag > 0
    _close(got, want)
    # ... whatever the sign of the zero imaginary parts
    got = _c_gain(scr_ref.AS_WRITTEN, complex(-32.0, -0.0), complex(128.0, -0.0), n, 0.0)
    assert got.real == 0.0 and got.imag > 0
    _close(got, want)
    # just off the negative real axis, on either side: the root follows the side
    for im in (1e-9, -1e-9):
        want = scr_ref.gain_from_sums(scr_ref.AS_WRITTEN, complex(-32.0, im), 128.0 + 0j, n, 0.0)
        got = _c_gain(scr_ref.AS_WRITTEN, complex(-32.0, im), 128.0 + 0j, n, 0.0)
        _close(got, want)
        assert math.copysign(1.0, got.imag) == math.copysign(1.0, want.imag) == (1.0 if im < 0 else -1.0)
    for power in (scr_ref.ABS2, scr_ref.AS_WRITTEN):
        # an all-zero clutter segment: gain 0
        assert _c_gain(power, 5.0 + 1j, 0j, n, 10.0) == 0j == scr_ref.gain_from_sums(power, 5.0 + 1j, 0j, n, 10.0)
        # an all-zero target row 1: P_s = eps, a large finite gain
        want = scr_ref.gain_from_sums(power, 0j, 64.0 + 0j, n, 20.0)
        got = _c_gain(power, 0j, 64.0 + 0j, n, 20.0)
        assert math.isfinite(got.real) and math.isfinite(got.imag) and got.real > 1e8
        _close(got, want)
        assert abs(got.real - math.sqrt(100.0 / scr_ref.EPS)) < 1e-6 * got.real
    # ABS2 ignores the imaginary sums: g = 12 / 3
    got = _c_gain(scr_ref.ABS2, complex(3.0, 99.0), complex(12.0, -7.0), n, 0.0)
    assert got.imag == 0.0 and abs(got.real - 2.0) < 1e-12
    _close(got, scr_ref.gain_from_sums(scr_ref.ABS2, complex(3.0, 99.0), complex(12.0, -7.0), n, 0.0))


def test_restatement_known_answers():
    """The restatement itself on a case small enough to do by hand."""
    simu = np.array([[1 + 0j, 1j, 2.0, 2.0], [3.0, 3.0, 1.0, 1.0]])
    clut = np.array([[2.0, 2.0, 1j, 1j, 9.0], [0.0, 0.0, 4.0, 4.0, 9.0]])       # one column wider
    segs, db = ((0, 2), (2, 2)), (10.0, 0.0)
    # ABS2, SCR 0: segment 0: P_s = 1, rows' P_echo = 4, 0 -> g = 40, 0; segment 1: P_s = 4, P_echo = 1, 16 -> g = 1/4, 4
    y, g = scr_ref.fun_SCR(simu, clut, 0.0, segs, db, scr_ref.ABS2)
    np.testing.assert_allclose(g, [[math.sqrt(40.0), 0.5], [0.0, 2.0]], rtol=1e-14)
    np.testing.assert_allclose(y, [[math.sqrt(40.0), math.sqrt(40.0) * 1j, 1.0, 1.0], [0, 0, 2.0, 2.0]], rtol=1e-14)
    np.testing.assert_allclose(scr_ref.fun_add_clutter(y, clut)[1], [0, 0, 6.0, 6.0], rtol=1e-14)
    # as written: segment 0 of row 1 squares to 1 + (-1) = 0 -> P_s = eps; segment 1's clutter row 1 to -1
    y, g = scr_ref.fun_SCR(simu, clut, 0.0, segs, db, scr_ref.AS_WRITTEN)
    assert abs(g[0, 0] - math.sqrt(40.0 / scr_ref.EPS)) < 1e-6 * abs(g[0, 0])
    np.testing.assert_allclose(g[:, 1], [0.5j, 2.0], rtol=1e-14)                 # sqrt(-1/4) = +j/2
    assert scr_ref.arg_margin(g[None, :, 1:]) == 0.0                             # g = -1/4 lies on the axis


def test_target_plan_geometry():
    from rsp import inject, presets
    spec = presets.v2(64, 1024)
    segs = [(s.in_start, s.in_len) for s in spec.segments]
    assert segs == [(0, 228), (228, 723), (951, 73)]
    dR = spec.radar["deltaR"]
    lam, prt = spec.radar["wavelength"], spec.radar["prt"]
    # 320 m: column 53 of every segment; 600 m: 100, past segment 3's 73 columns; 4200 m: 700, inside
    # segment 2 only, its 700-sample waveform cut to 23 columns by the segment's end; -5 m: nowhere
    Rg = np.array([320.0, 600.0, 4200.0, -5.0])
    Vg = np.array([-5.7, 12.0, -20.0, 3.0])
    plan = inject.target_plan(spec, Rg, Vg)
    assert plan.segments == segs and plan.batch == 4 and plan.seg_db == [0.0, 0.0, 0.0]
    assert round(320.0 / dR) == 53 and round(600.0 / dR) == 100 and round(4200.0 / dR) == 700
    np.testing.assert_array_equal(plan.delay, [[53, 53, 53, -1], [100, 100, -1, -1], [-1, 700, -1, -1], [-1, -1, -1, -1]])
    np.testing.assert_allclose(plan.dphi, 2 * np.pi * (2 * Vg / lam) * prt, rtol=1e-15)
    assert [len(w) for w in plan.wf_host] == [4, 200, 700] and list(plan.wf_off) == [0, 4, 204, 904]
    assert all(w.dtype == np.complex64 for w in plan.wf_host)
    np.testing.assert_array_equal(plan.wf_host[0], np.ones(4))
    assert abs(np.max(np.abs(plan.wf_host[2])) - 1.0) < 1e-6
    # r0 per segment: segment 2 measured from 300 m
    plan2 = inject.target_plan(spec, [320.0], [5.0], r0=[0.0, 300.0, 0.0])
    np.testing.assert_array_equal(plan2.delay, [[53, round(20.0 / dR), 53, -1]])
    # the materialised target: truncation at the segment's end, nothing where the delay is -1
    x = scr_ref.echo_simu(spec.P, spec.R, plan.segments, plan.wf_host, plan.delay, plan.dphi)
    assert np.count_nonzero(x[2, 0]) == 23 and np.count_nonzero(x[2, 0, 228 + 700:951]) == 23
    assert np.count_nonzero(x[3]) == 0
    assert np.count_nonzero(x[1, 5, :228]) == 4 and np.count_nonzero(x[1, 5, 951:]) == 0
    np.testing.assert_allclose(x[0, 7, 53], np.exp(1j * plan.dphi[0] * 7), rtol=1e-14)
    np.testing.assert_allclose(np.abs(x[0, :, 228 + 53]), np.abs(x[0, 0, 228 + 53]), rtol=1e-14)   # constant modulus over pulses
    # truth cells: the fixture formula of tests/test_gpu_score.py, the column through out_start - in_start
    t = plan.truth_cells(spec, 1)
    rows = [int(round(2 * v / lam * spec.P * prt)) + spec.P // 2 for v in Vg]
    np.testing.assert_array_equal(t[:, 0], rows)
    np.testing.assert_array_equal(t[:, 1], [228 + 53, 228 + 100, 228 + 700, 0])
    np.testing.assert_array_equal(t[:, 2], [0, 1, 0, 0])      # the gate: R > 400, 3 < |V| < 20; none without a target
    with pytest.raises(ValueError):
        inject.target_plan(spec, [1.0, 2.0], [1.0])

    leg = presets.legacy(48)
    assert [(s.in_start, s.in_len) for s in leg.segments] == list(scr_ref.LEGACY_SEGMENTS) == list(inject.LEGACY_SEGMENTS)
    assert tuple(inject.LEGACY_SEG_DB) == scr_ref.LEGACY_SEG_DB
    dRl = 2.99792458e8 / (2 * 25e6)
    pl = inject.target_plan(leg, [320.0, 81 * dRl, 82 * dRl, 4100.0], [5.0, 5.0, 5.0, 5.0])
    np.testing.assert_array_equal(pl.delay[:, :3], [[53, 53, 53], [81, 81, 81], [-1, 82, 82], [-1, -1, round(4100.0 / dRl)]])
    assert pl.delay[3, 2] == 684 and 684 + len(pl.wf_host[2]) > 707              # truncated by the row's end
    xl = scr_ref.echo_simu(leg.P, leg.R, pl.segments, pl.wf_host, pl.delay, pl.dphi)
    assert np.count_nonzero(xl[3, 0]) == np.count_nonzero(pl.wf_host[2][:707 - 684]) and xl.shape == (4, 48, 1031)
    assert np.count_nonzero(xl[1, 0, :82]) == 1                                   # four ones cut to one column
    with pytest.raises(ValueError):
        pl.truth_cells(presets.legacy(1536, 1031, concat=True), 1)
    nosh = presets.dmx_native()
    with pytest.raises(ValueError):
        inject.target_plan(nosh, [100.0], [5.0]).truth_cells(nosh, 0)
