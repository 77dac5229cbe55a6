"""The host-buffer entry points (rsp_pc_mtd_cfar, rsp_pc_mtd_cfar_f64, rsp_pc_mtd, rsp_cfar,
rsp_cfar_f64: the MEX drop-in) at ragged shapes, on every route of rsp_host.cpp, with every input
form and every output combination -- the table, the routes and the layout restatement are
tests/hostpath_cases.py's, held to rsp_hostplan.h without a GPU by tests/test_hostpath_cases_cpu.py.

Only layout work and exact conversions separate a host call from the device path, so every bar is
bit equality (np.array_equal):

  * the outputs equal hostpath_cases.expected_outputs of the device path (run_dev, cfar_dev) on the
    same context, fed the samples the device actually sees: the complex64 echo, the same fp16
    tensor, or -- for the C128 echo that is not float-representable (double noise with planted
    fp32 round-to-even ties and values that narrow to 0) -- echo.astype(complex64);
  * every output array lies inside a buffer of 0xA5 bytes with at least 4096 guard bytes on each
    side (the second call's arrays 8 bytes further in: 8- but not 16-byte aligned); the guards are
    intact after the call, an undelivered cell still holds 0xA5 bytes and fails the comparison;
  * the caller's input is unchanged;
  * every case runs twice back to back on one context with two different echoes and each call
    returns its own echo's result (no stale staging is read);
  * the device path itself is held, once per shape and input type, to fp64: pulse compression to
    test_gpu_pc_geometry.ref_pc, the RDM to mtd_ref of the pulse-compressed rows at the bars of
    test_gpu_mtd_instances (plane, maximum, every row and column within 1e-5), the flags to the C
    oracle fed the same RDM.

One line per case: HOST-SWEEP id shape route dtype layouts outs: ok.  The last test is the census:
per route, every (input dtype, input layout) and every (output layout, output type, number of
outputs) was visited.
"""
import ctypes as C

import numpy as np
import pytest

import hostpath_cases as hc
import mtd_ref as mr
from _util import MAX_TOL, NEAR_TOL, RDM_TOL, flag_mismatch, max_rel, oracle_flags_c, rel_err
from test_gpu_cfar_dispatch import cfar_obj
from test_gpu_mtd_instances import case_spec, rows_cols
from test_gpu_pc_geometry import ref_pc

pytestmark = pytest.mark.gpu

CFAR_T = 1.5          # low enough that noise alone sets flags all over the plane
VISITED, ATTEMPTED = set(), set()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _engine(shape):
    from rsp.engine import Engine
    return Engine(case_spec(shape.pin, shape.R, nfft=shape.nfft, beams=shape.beams), device=0)


def _cfar():
    return cfar_obj(mr.W32 + mr.W32, CFAR_T, 0, 20, [], (0, 0))


def _echo_shape(shape, batch):
    return (batch, shape.pin, shape.R) if shape.beams == 1 else (batch, shape.beams, shape.pin, shape.R)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _dev(torch, eng, shape, src, nout, cf):
    """The device path on `src` (complex64, or fp16 I/Q): (rdm, flag, flagV) row-major, None where
    the call has no such output."""
    batch = src.shape[0]
    oshape = (batch, shape.V, shape.R)
    rdm = torch.empty(oshape, dtype=torch.float32, device="cuda")
    flag = torch.empty(oshape, dtype=torch.uint8, device="cuda") if nout >= 2 else None
    fv = torch.empty(oshape, dtype=torch.uint8, device="cuda") if nout >= 3 else None
    eng.run_dev(torch.from_numpy(src).cuda(), rdm=rdm, flag=flag, flagV=fv, cfar=cf if nout >= 2 else None)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() if t is not None else None for t in (rdm, flag, fv))


class Inputs:
    """The two echoes of one (shape, batch): A, complex64 noise, and B, the narrowing of a complex128
    echo that is not float-representable -- in every form a caller can pass, with the device
    path's outputs for each."""

    def __init__(self, torch, eng, shape, batch, cf):
        self.torch, self.eng, self.shape, self.cf = torch, eng, shape, cf
        es = _echo_shape(shape, batch)
        seed = hc.SEED + 1000 * batch + shape.pin
        d = hc.double_echo(es, seed + 1)
        self.forms = [hc.echo_variants(hc.noise_echo(es, seed)), hc.echo_variants(d.astype(np.complex64))]
        self.forms[1][hc.C128, hc.ROW] = d
        self.forms[1][hc.C128, hc.COL] = hc.column_major_c128(d)
        assert not np.array_equal(d.astype(np.complex64).astype(np.complex128), d)
        self.refs = {}

    def ref(self, call, dtype, nout):
        key = (call, dtype == hc.F16, nout)
        if key not in self.refs:
            src = self.forms[call][hc.F16 if dtype == hc.F16 else hc.C64, hc.ROW]
            out = _dev(self.torch, self.eng, self.shape, src, nout, self.cf)
            assert np.isfinite(out[0]).all() and out[0].any()
            if nout >= 2:
                assert out[1].any() and not out[1].all() and out[1].max() == 1
            self.refs[key] = out
        return self.refs[key]


def _host_call(eng, c, shape, echo, outs, cf):
    """The case's entry point on `echo` into the arrays `outs` (rdm[, flag[, flagV]])."""
    from rsp import _capi as capi
    lib = eng.lib
    cp = cf.to_c() if c.nout >= 2 else None
    o = list(outs) + [None] * (3 - len(outs))
    if c.entry == "pc_mtd":
        rc = lib.rsp_pc_mtd(eng.ctx, _ptr(echo), c.dtype, c.layout, shape.pin, shape.R, c.batch, _ptr(o[0]), c.out_layout)
    else:
        fn = lib.rsp_pc_mtd_cfar_f64 if c.f64 else lib.rsp_pc_mtd_cfar
        rc = fn(eng.ctx, _ptr(echo), c.dtype, c.layout, shape.pin, shape.R, c.batch, C.byref(cp) if cp is not None else None,
                _ptr(o[0]), c.out_layout, _ptr(o[1]), _ptr(o[2]))
    capi.check(rc, eng.ctx)


def _run_case(eng, c, shape, inputs, cf):
    oshape = (c.batch, shape.V, shape.R) if c.out_layout == hc.ROW else (c.batch, shape.R, shape.V)
    dts = ([np.float64] * 3 if c.f64 else [np.float32, np.uint8, np.uint8])[:c.nout]
    eng.set_host_pipeline(c.chunk, 0)
    for call in (0, 1):
        echo = inputs.forms[call][c.dtype, c.layout]
        before = echo.copy()
        want = hc.expected_outputs(*inputs.ref(call, c.dtype, c.nout), c.out_layout, c.f64)
        lead = hc.GUARD + 8 * call
        bufs = [hc.guarded(oshape, dt, lead) for dt in dts]
        _host_call(eng, c, shape, echo, [v for _, v in bufs], cf)
        for k, ((raw, got), w) in enumerate(zip(bufs, want)):
            what = "%s call %d output %d" % (c.id, call, k)
            assert hc.guards_intact(raw, got, lead), what + ": a guard byte was written"
            assert got.dtype == w.dtype and got.shape == w.shape
            if not np.array_equal(got, w):
                bad = np.argwhere(got != w)
                raise AssertionError("%s: %d of %d cells differ, first at %s, last at %s"
                                     % (what, len(bad), got.size, tuple(int(i) for i in bad[0]), tuple(int(i) for i in bad[-1])))
        assert np.array_equal(echo.view(np.uint8), before.view(np.uint8)), c.id + ": the caller's echo was changed"


@pytest.mark.parametrize("group", hc.GROUPS)
def test_host_sweep(torch_cuda, group):
    cases = [c for c in hc.CASES if c.group == group]
    ATTEMPTED.add(group)
    shape = hc.SHAPES[cases[0].shape]
    eng = _engine(shape)
    cf = _cfar()
    inputs = {}
    try:
        for c in cases:
            r = hc.route(c)
            assert r["route"] == c.want
            if c.batch not in inputs:
                inputs[c.batch] = Inputs(torch_cuda, eng, shape, c.batch, cf)
            _run_case(eng, c, shape, inputs[c.batch], cf)
            VISITED.add(c.id)
            print("HOST-SWEEP %s %dx%dx%d beams %d route %s (%d chunks) %s in %s out %s %s outs %d: ok"
                  % (c.id, c.batch, shape.pin, shape.R, shape.beams, r["route"], r["nk"], hc.DTYPE_NAME[c.dtype],
                     hc.LAYOUT_NAME[c.layout], hc.LAYOUT_NAME[c.out_layout], "f64" if c.f64 else "f32/u8", c.nout))
    finally:
        eng.close()


@pytest.mark.parametrize("sid,batch", hc.CFAR_CALLS)
def test_cfar_entry_points(torch_cuda, sid, batch):
    """rsp_cfar and rsp_cfar_f64 on the device path's RDM, both layouts, with and without flagV_out,
    two RDMs back to back: the flags of rsp_cfar_dev on the same planes, bit for bit."""
    torch = torch_cuda
    from rsp import _capi as capi
    shape = hc.SHAPES[sid]
    eng = _engine(shape)
    cf = _cfar()
    cp = cf.to_c()
    V, R = shape.V, shape.R
    try:
        planes = []
        for call in (0, 1):
            echo = hc.noise_echo(_echo_shape(shape, batch), hc.SEED + 77 + call + batch)
            rdm = _dev(torch, eng, shape, echo, 1, None)[0]
            d_rdm = torch.from_numpy(rdm).cuda()
            d_flag, d_fv = torch.empty_like(d_rdm, dtype=torch.uint8), torch.empty_like(d_rdm, dtype=torch.uint8)
            eng.cfar_dev(d_rdm, d_flag, d_fv, cfar=cf)
            torch.cuda.synchronize()
            flag, fv = d_flag.cpu().numpy(), d_fv.cpu().numpy()
            assert flag.any() and not flag.all() and fv.any() and not fv.all()
            planes.append((rdm, flag, fv))
        for lay in (hc.ROW, hc.COL):
            oshape = (batch, V, R) if lay == hc.ROW else (batch, R, V)
            for f64 in (False, True):
                for want_fv in (True, False):
                    for call, (rdm, flag, fv) in enumerate(planes):
                        x = hc.expected_outputs(rdm, None, None, lay, f64)[0]
                        before = x.copy()
                        want = hc.expected_outputs(None, flag, fv if want_fv else None, lay, f64)
                        lead = hc.GUARD + 8 * call
                        bufs = [hc.guarded(oshape, np.float64 if f64 else np.uint8, lead) for _ in want]
                        o = [v for _, v in bufs] + [None]
                        fn = eng.lib.rsp_cfar_f64 if f64 else eng.lib.rsp_cfar
                        capi.check(fn(eng.ctx, _ptr(x), lay, V, R, batch, C.byref(cp), _ptr(o[0]), _ptr(o[1])), eng.ctx)
                        what = "%s b%d %s %s flagV %d call %d" % (sid, batch, hc.LAYOUT_NAME[lay], "f64" if f64 else "u8",
                                                                  want_fv, call)
                        for (raw, got), w in zip(bufs, want):
                            assert hc.guards_intact(raw, got, lead), what
                            assert np.array_equal(got, w), what
                        assert np.array_equal(x, before), what
                        print("HOST-SWEEP cfar %s: ok" % what)
    finally:
        eng.close()


@pytest.mark.parametrize("sid", sorted(hc.SHAPES))
def test_device_path_against_fp64(torch_cuda, sid):
    """The reference of this sweep is the device path; here it is held to fp64 on the sweep's own
    contexts and echoes, complex64 and fp16: pulse compression to ref_pc (the PC sweep's bars), the
    RDM to mtd_ref of the GPU's pulse-compressed rows (the MTD sweep's bars), the flags to the C
    oracle fed the GPU's RDM."""
    torch = torch_cuda
    shape = hc.SHAPES[sid]
    eng = _engine(shape)
    cf = _cfar()
    batch, nb, pin, R, V = 2, shape.beams, shape.pin, shape.R, shape.V
    try:
        forms = hc.echo_variants(hc.noise_echo(_echo_shape(shape, batch), hc.SEED + shape.pin))
        w, zb = mr.slow_time_window(mr.KAISER, pin), mr.zero_band(V)
        for dtype in (hc.C64, hc.F16):
            src = forms[dtype, hc.ROW]
            x = (src[..., 0].astype(np.float64) + 1j * src[..., 1].astype(np.float64)) if dtype == hc.F16 else src.astype(np.complex128)
            d_pc = torch.empty((batch * nb, pin, R), dtype=torch.complex64, device="cuda")
            d_src = torch.from_numpy(src).cuda()
            eng.pc_dev(d_src.view((batch * nb, pin, R) + ((2,) if dtype == hc.F16 else ())), d_pc)
            torch.cuda.synchronize()
            pc = d_pc.cpu().numpy().astype(np.complex128)
            want_pc = ref_pc(eng.spec, x.reshape(batch * nb * pin, R)).reshape(pc.shape)
            epc = (rel_err(pc.view(np.float64), want_pc.view(np.float64)), float(np.abs(pc - want_pc).max() / np.abs(want_pc).max()))
            assert epc[0] < RDM_TOL and epc[1] < MAX_TOL, (sid, epc)
            rdm, flag, fv = _dev(torch, eng, shape, src, 3, cf)
            pcb = pc.reshape((batch, pin, R) if nb == 1 else (batch, nb, pin, R))
            worst = np.zeros(4)
            for b in range(batch):
                o = mr.mtd_ref(pcb[b], w, V, 1, zb, 0, nb)
                want = o[0] if nb == 2 else o
                fig = (rel_err(rdm[b], want), max_rel(rdm[b], want)) + rows_cols(rdm[b], want, zb)
                worst = np.maximum(worst, fig)
                assert fig[0] < RDM_TOL and fig[1] < MAX_TOL and fig[2] < RDM_TOL and fig[3] < RDM_TOL, (sid, b, fig)
            assert flag.max() <= 1 and fv.max() <= 1
            oflag, oflagV, amb = oracle_flags_c(rdm.astype(np.float64), cf, NEAR_TOL)
            hard, soft = flag_mismatch(flag, oflag, amb)
            hardv, softv = flag_mismatch(fv, oflagV, amb)
            assert hard == 0 and hardv == 0 and soft <= int(amb.sum()) and softv <= int(amb.sum()), (sid, hard, hardv)
            assert oflag.any() and oflagV.any()
            print("HOST-SWEEP device path %s %s: pc rel %.2e max %.2e; rdm plane %.2e max %.2e row %.2e col %.2e; "
                  "flags %d / %d, mask %d, soft %d+%d" % ((sid, hc.DTYPE_NAME[dtype]) + epc + tuple(worst)
                                                         + (int(oflag.sum()), int(oflagV.sum()), int(amb.sum()), soft, softv)))
    finally:
        eng.close()


def test_sweep_visited_every_route_with_every_form():
    """Per route: every (input dtype, input layout) and every (output layout, output type, number
    of outputs), by route() of the table -- and, when the whole sweep ran in this session, of the
    cases it ran to their end."""
    assert hc.census(hc.CASES) == hc.expected_census()
    if ATTEMPTED == set(hc.GROUPS):
        assert hc.census([c for c in hc.CASES if c.id in VISITED]) == hc.expected_census()
        assert VISITED == {c.id for c in hc.CASES}
    for r in hc.ROUTES:
        ins, outs = hc.census(hc.CASES)[r]
        print("HOST-SWEEP census route %-5s: %d cases, %d input forms, %d output combinations"
              % (r, sum(1 for c in hc.CASES if hc.route(c)["route"] == r), len(ins), len(outs)))
