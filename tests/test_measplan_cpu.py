"""The hit-list geometry of the measurement and of the condensation's plot list
(radar-signal-process_amd/csrc/rsp_measplan.h: meas_plan, used by launch_e and launch_hit_list)
on the CPU.  A stand-alone program compares it with geometries worked out by hand: the rows of
tests/measure_cases.py and R = 255/256/272, 1024/1025, 16384/16400.  rsp_measure_plan, the
read-only entry point over the same function, needs no GPU either: its answers and its refusals
are checked through ctypes with made-up flag addresses (it never dereferences them)."""
import ctypes as C
import os
import subprocess

import measure_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "measplan_check.cpp")
INC = os.path.join(ROOT, "radar-signal-process_amd", "csrc")
ADDR = 0x7f0000001000


def test_hand_worked_geometries(tmp_path):
    exe = str(tmp_path / "measplan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC, SRC, "-o", exe], check=True,
                   capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def _params(e=2, M0=1, ri=8, vi=4, ld=0, cs=0):
    from rsp import _capi
    p = _capi.rsp_measure_params()
    p.extra_dots, p.r_interp, p.v_interp, p.mtd0_num = e, ri, vi, M0
    p.ld, p.cpi_stride = ld, cs
    return p


def test_entry_point_reports_the_table():
    """rsp_measure_plan on every row of the case table, with an aligned base address plus the row's
    window column: the row's stated plan."""
    from rsp import _capi
    lib = _capi.load_library()
    assert "rsp_measure_plan" in _capi.EXPORTS
    for c in mc.CASES:
        p = _params(c.e, c.M0, c.interp[0], c.interp[1], c.ld, c.cs)
        out = _capi.rsp_measure_plan_t()
        rc = lib.rsp_measure_plan(None, C.c_void_p(ADDR + 64 + c.col0), c.V, c.R, c.batch, C.byref(p), C.byref(out))
        assert rc == 0, c.id
        got = dict(wide=bool(out.wide), G=out.groups, S=out.slices, rows=out.rows, q=out.q, passes=out.passes)
        assert got == c.plan, c.id
        assert out.cw == (16 if out.wide else 1) and out.bands == 1


def test_entry_point_refusals():
    """What rsp_motion_measure_dev's own validation returns, in its order, and `out` untouched."""
    from rsp import _capi
    lib = _capi.load_library()
    ARG, UNSUP = _capi.RSP_ERR_ARG, _capi.RSP_ERR_UNSUPPORTED
    flag = C.c_void_p(ADDR)

    def call(p, V=40, R=256, batch=3, flag=flag, out=True):
        o = _capi.rsp_measure_plan_t()
        o.wide = o.groups = o.passes = -5
        rc = lib.rsp_measure_plan(None, flag, V, R, batch, None if p is None else C.byref(p),
                                  C.byref(o) if out else None)
        if rc:
            assert (o.wide, o.groups, o.passes) == (-5, -5, -5)
        return rc

    def msg():
        return lib.rsp_last_error(None).decode()

    assert call(_params()) == 0
    assert call(None) == ARG and call(_params(), flag=None) == ARG and call(_params(), out=False) == ARG
    assert call(_params(), batch=-1) == ARG
    assert call(_params(e=0)) == UNSUP and "extra_dots" in msg()
    assert call(_params(e=5)) == UNSUP
    for ri, vi in ((0, 4), (65, 4), (8, 0), (8, 65)):
        assert call(_params(ri=ri, vi=vi)) == ARG and "interpolation" in msg()
    assert call(_params(), V=0) == ARG and call(_params(), R=0) == ARG and "bad shape" in msg()
    assert call(_params(e=2), R=4) == ARG and "fewer" in msg()             # R < 2e+1
    assert call(_params(e=2), R=5, V=8) == 0                                # R == 2e+1, V - 2*M0 - 1 == 2e+1
    assert call(_params(e=2, M0=2), V=9, R=5) == ARG and "fewer" in msg()   # 9 - 4 - 1 = 4 < 5
    assert call(_params(M0=-1)) == ARG
    assert call(_params(ld=255)) == ARG and "row pitch" in msg()
    assert call(_params(ld=304, cs=39 * 304 + 255)) == ARG and "row pitch" in msg()
    assert call(_params(ld=304, cs=39 * 304 + 256)) == 0
    assert call(_params(), batch=0) == 0
