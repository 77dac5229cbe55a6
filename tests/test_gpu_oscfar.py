"""Ordered-statistic CFAR on the GPU (rsp_os_cfar_dev, csrc/rsp_oscfar.hip) against the sorted
restatement tests/oscfar_ref.py.  Every comparison is exact equality of whole flag and flagV
planes: the rule is stated in fp32, so there is no tie band and no cell is left out.
tests/test_oscfar_cpu.py audits the scenes (each carries a detection on every edge a kernel could
ignore) and holds the restatement to a counting form, an fp64 form and the existing oracle.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oscfar_ref as osr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def oc():
    from rsp.oscfar import OsCfar
    o = OsCfar(0)
    yield o
    o.close()


def _cfar(p):
    from rsp import presets
    return presets.Cfar(refR=p.refR, saveR=p.saveR, TR=p.TR, methodR=p.method, refV=p.refV, saveV=p.saveV, TV=p.TV,
                        methodV=p.method, M0=p.M0, rFlag=p.rFlag, zero_v_div=p.zero_v_div, segments=list(p.segments))


def _detect(oc, d_x, p, **kw):
    flag, flagV = oc.detect_dev(d_x, _cfar(p), (p.kV, p.kR), (p.union, p.union), **kw)
    return flag.cpu().numpy(), flagV.cpu().numpy()


def _same(got, want, tag):
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert bad.size == 0, (tag, len(bad), bad[:4].tolist())


_REF = {}


def _want(shape, case):
    """The restatement's planes of one sweep case, computed once."""
    key = (shape.name,) + tuple(case)
    if key not in _REF:
        p = shape.params(*case)
        r = [osr.os_cfar(x, p) for x in osr.scene(shape)]
        _REF[key] = (np.stack([q["flag"] for q in r]), np.stack([q["flagV"] for q in r]))
    return _REF[key]


@pytest.mark.parametrize("shape", osr.SHAPES, ids=[s.name for s in osr.SHAPES])
def test_shape_sweep(oc, shape):
    """Per-side GO, per-side SO and union, each at k = 1, the middle and the largest rank, with rFlag
    0 and 1, on the four shapes (none / one inner / three segments; the 332-row plane with its
    zero_v_div band and the block of exact zeros; 2048 rows in a batch of 2)."""
    import torch
    d_x = torch.from_numpy(np.array(osr.scene(shape))).cuda()
    flags = 0
    for case in osr.cases(shape):
        p = shape.params(*case)
        flag, flagV = _detect(oc, d_x, p)
        want, wantV = _want(shape, case)
        _same(flagV, wantV, (case, "flagV"))
        _same(flag, want, (case, "flag"))
        flags += int(want.sum())
    assert flags > 0


def test_every_plan_instance_is_reached(oc):
    """The Doppler kernel's tile width is sized by V alone (2^1 .. 2^6 columns for V <= 4096) and the
    range stage is a gather or absent: the sweep's shapes and three narrow planes take every one, as
    rsp_os_cfar_plan reports them, and the narrow planes' flags are the restatement's too."""
    import torch
    from rsp import _capi as capi
    seen_v, seen_r = set(), set()
    for shape in osr.SHAPES + osr.TILE_SHAPES:
        for rf in (0, 1):
            p = shape.params(osr.UNION, shape.ref, rf)
            plan = oc.plan(shape.V, shape.R, shape.batch, _cfar(p), (p.kV, p.kR), (True, True))
            seen_v.add(plan["v_tile_log2"])
            seen_r.add(plan["r_stage"])
            assert plan["r_tiles"] == (1 if rf else 0) and plan["r_halo"] == (shape.ref + shape.save + 2 if rf else 0)
            if shape in osr.TILE_SHAPES:
                x = osr.scene(shape)
                flag, flagV = _detect(oc, torch.from_numpy(np.array(x)).cuda(), p)
                r = osr.os_cfar(x[0], p)
                _same(flagV[0], r["flagV"], (shape.name, rf, "flagV"))
                _same(flag[0], r["flag"], (shape.name, rf, "flag"))
                assert r["flag"].sum() > 0
    assert seen_v == {1, 2, 3, 4, 5, 6}
    assert seen_r == {capi.RSP_OS_R_NONE, capi.RSP_OS_R_GATHER}


def test_wide_rows_take_more_than_one_range_tile(oc):
    """A row of 2300 columns is three range tiles (1024 columns each, the last one short): a hit next
    to a tile edge is resolved across it."""
    import torch
    shape = osr.Shape("24x2300", 24, 2300, 3, 2, 1, 0)
    rng = np.random.default_rng(9)
    x = rng.rayleigh(np.sqrt(2.0 / np.pi), (24, 2300)).astype(np.float32)
    for i, c in enumerate((1022, 1023, 1024, 1025, 2047, 2048, 2299)):
        x[3 + 2 * i, c] = 40.0 + i
        x[3 + 2 * i, c - 1] = 39.0
    for form, k in ((osr.GO, 2), (osr.UNION, 4)):
        p = shape.params(form, k, 1)
        assert oc.plan(24, 2300, 1, _cfar(p), (k, k), (p.union, p.union))["r_tiles"] == 3
        flag, flagV = _detect(oc, torch.from_numpy(x).cuda(), p)
        r = osr.os_cfar(x, p)
        _same(flagV[0], r["flagV"], (form, "flagV"))
        _same(flag[0], r["flag"], (form, "flag"))
        assert r["moved"].any()


def test_window_of_wider_planes(oc):
    """A 96 x 130 window at column 7 of ld = 160 planes with a padded CPI stride: the amplitudes
    outside the window are 3e30 and the flag bytes outside it 0xAA; the window's flags are the
    restatement's and no byte outside it changes."""
    import torch
    from rsp import _capi as capi
    w = osr.WIN
    V, R, c0, ld, cs, B = w["V"], w["R"], w["col0"], w["ld"], w["cs"], w["batch"]
    shape = osr.Shape("win", V, R, w["ref"], w["save"], w["M0"], w["nseg"], batch=B)
    x = osr.scene(shape)
    amp = np.full(B * cs + 64, 3.0e30, np.float32)
    inside = np.zeros(B * cs + 64, bool)
    for b in range(B):
        for v in range(V):
            o = b * cs + v * ld + c0
            amp[o:o + R] = x[b, v]
            inside[o:o + R] = True
    d_amp = torch.from_numpy(amp).cuda()
    for case in ((osr.GO, 3, 1), (osr.UNION, 7, 1), (osr.SO, 5, 0)):
        p = shape.params(*case)
        d_flag = torch.full((B * cs + 64,), 0xAA, dtype=torch.uint8, device="cuda")
        d_flagV = torch.full((B * cs + 64,), 0xAA, dtype=torch.uint8, device="cuda")
        op = capi.rsp_os_params()
        op.kV = op.kR = p.kV
        op.unionV = op.unionR = int(p.union)
        op.ld, op.cpi_stride = ld, cs
        cp = _cfar(p).to_c()
        st = torch.cuda.current_stream().cuda_stream
        capi.check(oc.lib.rsp_os_cfar_dev(oc.ctx, d_amp.data_ptr() + 4 * c0, V, R, B, C.byref(cp), C.byref(op),
                                          d_flag.data_ptr() + c0, d_flagV.data_ptr() + c0, C.c_void_p(st)), oc.ctx)
        flag, flagV = d_flag.cpu().numpy(), d_flagV.cpu().numpy()
        assert (flag[~inside] == 0xAA).all() and (flagV[~inside] == 0xAA).all()
        for b in range(B):
            r = osr.os_cfar(x[b], p)
            rows = (b * cs + np.arange(V)[:, None] * ld + c0 + np.arange(R)[None, :])
            _same(flagV[rows], r["flagV"], (case, b, "flagV"))
            _same(flag[rows], r["flag"], (case, b, "flag"))
            assert r["flag"].sum() > 0


def test_scratch_flagV_equals_callers(oc):
    """With rFlag = 1 and no d_flagV the Doppler flags go to the context's scratch: same flag plane."""
    import torch
    shape = osr.SHAPES[1]
    case = (osr.UNION, 5, 1)
    p = shape.params(*case)
    d_x = torch.from_numpy(np.array(osr.scene(shape))).cuda()
    d_flag = torch.empty(d_x.shape, dtype=torch.uint8, device="cuda")
    op = osr_params(p)
    cp = _cfar(p).to_c()
    st = torch.cuda.current_stream().cuda_stream
    from rsp import _capi as capi
    capi.check(oc.lib.rsp_os_cfar_dev(oc.ctx, d_x.data_ptr(), shape.V, shape.R, shape.batch, C.byref(cp), C.byref(op),
                                      d_flag.data_ptr(), None, C.c_void_p(st)), oc.ctx)
    _same(d_flag.cpu().numpy(), _want(shape, case)[0], "flag")
    assert oc.plan(shape.V, shape.R, 1, _cfar(p), (5, 5), (True, True), flagV=False)["scratch_flagV"] == 1


def osr_params(p):
    from rsp.oscfar import os_params
    return os_params((p.kV, p.kR), (p.union, p.union))


@pytest.mark.parametrize("form", [osr.GO, osr.SO])
def test_rank_one_of_one_cell_equals_rsp_cfar_dev(oc, form):
    """ref = 1, k = 1, T = 4: the mean of a one-cell window is its first smallest cell and every
    product is exact, so rsp_os_cfar_dev and rsp_cfar_dev give the same bytes (rFlag 1, three
    segments)."""
    import torch
    V, R, save, M0 = 64, 130, 2, 2
    segs = osr.cfar_scene.layout(R, 1 + save, 3)
    x = np.array(osr.scene(osr.SHAPES[2])[:, :V, :R])
    p = osr.Params(1, save, 1, save, M0, tuple(segs), 0, 4.0, 4.0, form, 1, 1, 1)
    d_x = torch.from_numpy(x).cuda()
    flag, flagV = _detect(oc, d_x, p)
    d_f = torch.empty(d_x.shape, dtype=torch.uint8, device="cuda")
    d_fv = torch.empty(d_x.shape, dtype=torch.uint8, device="cuda")
    cp = _cfar(p).to_c()
    from rsp import _capi as capi
    capi.check(oc.lib.rsp_cfar_dev(oc.ctx, d_x.data_ptr(), V, R, x.shape[0], C.byref(cp), d_f.data_ptr(),
                                   d_fv.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), oc.ctx)
    _same(flagV, d_fv.cpu().numpy(), "flagV")
    _same(flag, d_f.cpu().numpy(), "flag")
    assert flag.sum() > 0 and not np.array_equal(flag, flagV)


def test_masking(oc):
    """Two lines of 40 and 45, saveV + 2 rows apart in one column (ref 5 / guard 7 / T 7): the
    greatest-of cell-averaging detector flags neither in flagV, the union k = 7 ordered statistic
    flags both."""
    import torch
    from rsp import _capi as capi
    x, a, b = osr.masking_scene()
    V, R = x.shape
    d_x = torch.from_numpy(x[None]).cuda()
    p = osr.Params(form=osr.UNION, kV=7, kR=7, **osr.MASK_PARAMS)
    d_f = torch.empty(d_x.shape, dtype=torch.uint8, device="cuda")
    d_fv = torch.empty(d_x.shape, dtype=torch.uint8, device="cuda")
    cp = _cfar(osr.Params(form=osr.GO, **osr.MASK_PARAMS)).to_c()
    capi.check(oc.lib.rsp_cfar_dev(oc.ctx, d_x.data_ptr(), V, R, 1, C.byref(cp), d_f.data_ptr(), d_fv.data_ptr(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), oc.ctx)
    ca = d_fv.cpu().numpy()[0]
    assert ca[a] == 0 and ca[b] == 0
    _, flagV = _detect(oc, d_x, p)
    assert flagV[0][a] == 1 and flagV[0][b] == 1
    _same(flagV[0], osr.os_cfar(x, p)["flagV"], "flagV")


def test_batch_and_run_determinism(oc):
    """Batch 5 equals the five CPIs one by one, and a second run equals the first."""
    import torch
    shape = osr.Shape("det", 64, 70, 5, 7, 2, 1, batch=5)
    x = np.array(osr.scene(shape))
    d_x = torch.from_numpy(x).cuda()
    for case in ((osr.GO, 1, 1), (osr.UNION, 7, 1)):   # at k = 1 the floor itself fires: five different planes
        p = shape.params(*case)
        flag, flagV = _detect(oc, d_x, p)
        flag2, flagV2 = _detect(oc, d_x, p)
        _same(flag2, flag, "second run")
        _same(flagV2, flagV, "second run, flagV")
        for b in range(5):
            f1, fv1 = _detect(oc, d_x[b:b + 1], p)
            _same(f1[0], flag[b], ("alone", b))
            _same(fv1[0], flagV[b], ("alone", b, "flagV"))
        assert flag.sum() > 0 and (case[1] > 1 or len({flag[b].tobytes() for b in range(5)}) == 5)


def test_error_paths(oc):
    """k = 0, k > ref per side, k > 2 ref union, T <= 0, a band shorter than 2 (guard + ref), ref = 33
    and a null os: the stated code, a message, and nothing launched (the flag bytes stay as set)."""
    import torch
    from rsp import _capi as capi
    V, R = 96, 40
    d_x = torch.ones((1, V, R), dtype=torch.float32, device="cuda")
    d_f = torch.full((1, V, R), 0xAA, dtype=torch.uint8, device="cuda")
    d_fv = torch.full((1, V, R), 0xAA, dtype=torch.uint8, device="cuda")
    base = dict(refV=5, saveV=7, refR=5, saveR=7, M0=2, TV=4.0, TR=4.0, rFlag=1)

    def call(kw=None, k=(3, 3), union=(0, 0), null_os=False, ctx=oc.ctx):
        cp = _cfar(osr.Params(**dict(base, **(kw or {})))).to_c()
        op = capi.rsp_os_params()
        op.kV, op.kR, op.unionV, op.unionR = k[0], k[1], union[0], union[1]
        rc = oc.lib.rsp_os_cfar_dev(ctx, d_x.data_ptr(), V, R, 1, C.byref(cp), None if null_os else C.byref(op),
                                    d_f.data_ptr(), d_fv.data_ptr(), None)
        return rc, (oc.lib.rsp_last_error(ctx) or b"").decode()

    want = [
        (dict(k=(0, 3)), capi.RSP_ERR_ARG, "kV"),
        (dict(k=(3, 0)), capi.RSP_ERR_ARG, "kR"),
        (dict(k=(6, 3)), capi.RSP_ERR_ARG, "kV"),
        (dict(k=(3, 6)), capi.RSP_ERR_ARG, "kR"),
        (dict(k=(11, 3), union=(1, 1)), capi.RSP_ERR_ARG, "kV"),
        (dict(k=(3, 11), union=(1, 1)), capi.RSP_ERR_ARG, "kR"),
        (dict(kw=dict(TV=0.0)), capi.RSP_ERR_ARG, "TV"),
        (dict(kw=dict(TR=-1.0)), capi.RSP_ERR_ARG, "TR"),
        (dict(kw=dict(TV=float("inf"))), capi.RSP_ERR_ARG, "TV"),
        (dict(kw=dict(M0=36)), capi.RSP_ERR_CFAR_WINDOW, "Doppler"),      # 23 band rows < 24
        (dict(kw=dict(segments=((0, 20), (20, 40)))), capi.RSP_ERR_CFAR_WINDOW, "segment"),
        (dict(kw=dict(refV=33, saveV=1), k=(3, 3)), capi.RSP_ERR_UNSUPPORTED, "ref"),
        (dict(null_os=True), capi.RSP_ERR_ARG, "os"),
    ]
    for kw, code, word in want:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    # the arguments are checked before the context is looked at
    rc, msg = call(k=(0, 3), ctx=None)
    assert rc == capi.RSP_ERR_ARG and "kV" in msg
    torch.cuda.synchronize()
    assert (d_f.cpu().numpy() == 0xAA).all() and (d_fv.cpu().numpy() == 0xAA).all()
    rc, _ = call()                       # and the same buffers with good arguments are written
    torch.cuda.synchronize()
    assert rc == capi.RSP_OK and (d_f.cpu().numpy() != 0xAA).all() and (d_fv.cpu().numpy() != 0xAA).all()


def test_profile_ids(oc):
    """The two launches are timed under rsp_profile as the kernel ids appended to the list."""
    import torch
    from rsp import _capi as capi
    shape = osr.SHAPES[0]
    p = shape.params(osr.GO, 1, 1)
    d_x = torch.from_numpy(np.array(osr.scene(shape))).cuda()
    capi.check(oc.lib.rsp_profile(oc.ctx, 1), oc.ctx)
    _detect(oc, d_x, p)
    ms = (C.c_double * capi.RSP_NKERNELS)()
    n = (C.c_int64 * capi.RSP_NKERNELS)()
    capi.check(oc.lib.rsp_profile_read_n(oc.ctx, ms, n, capi.RSP_NKERNELS), oc.ctx)
    capi.check(oc.lib.rsp_profile(oc.ctx, 0), oc.ctx)
    assert list(n) == [0, 0, 0, 0, 1, 1] and ms[4] > 0 and ms[5] > 0
    assert capi.KERNEL_NAMES[4:] == ("os_v_kernel", "os_r_kernel")


# ---------------------------------------------------------------- the DMX loop
@pytest.fixture(scope="module")
def dmx():
    import torch
    from rsp.dmx import DmxFrameProcessor
    echo = np.load(os.path.join(GOLDEN, "dmx_32x512.npz"))["echo"].astype(np.complex64)
    P, R = echo.shape
    proc = DmxFrameProcessor(freInd=2, P=P, R=R)
    e = np.stack([np.stack([echo, 0.7 * echo]), np.stack([echo[::-1], 0.6 * echo[::-1]])]).astype(np.complex64)
    yield proc, torch.from_numpy(e).cuda()
    proc.close()


def test_dmx_frame_processor_detector(dmx, oc):
    """process_dev(detector=...): flag and flagV are OsCfar.detect_dev on the call's own sum plane
    with the preset's window and segments; sum and diff are those of the call without a detector;
    the measurement runs on the new flags."""
    proc, echo = dmx
    # 32 pulses in a 2048-point Doppler transform: a line is 64 rows wide, far wider than the window,
    # so only a threshold near the 7th smallest neighbour itself flags anything on this input
    det = dict(k=(7, 7), union=(True, True), T=(1.25, 1.25))
    out = proc.process_dev(echo, 3, detector=det)
    base = proc.process_dev(echo, 3)
    for k in ("sum", "diff"):
        assert np.array_equal(out[k].cpu().numpy(), base[k].cpu().numpy()), k
    import dataclasses
    cf = dataclasses.replace(proc.cfar, TV=1.25, TR=1.25)
    flag, flagV = oc.detect_dev(out["sum"], cf, (7, 7), (True, True))
    _same(out["flag"].cpu().numpy(), flag.cpu().numpy(), "flag")
    _same(out["flagV"].cpu().numpy(), flagV.cpu().numpy(), "flagV")
    f = out["flag"].cpu().numpy()
    assert f.sum() > 0 and not np.array_equal(f, base["flag"].cpu().numpy())
    ps = proc.spec.cfar_segments[0][1]
    for part, cols in (("short", slice(0, ps)), ("long", slice(ps, None))):
        count = out[(part, "flag")][2].cpu().numpy()
        assert np.array_equal(count[:, 0], f[:, :, cols].sum(axis=(1, 2)))
    with pytest.raises(TypeError):
        proc.process_dev(echo, 3, detector=dict(k=(7, 7), rank=3))


# ---------------------------------------------------------------- the score sweeps
@pytest.fixture(scope="module")
def chain():
    import torch
    from rsp import presets, synth
    from rsp.engine import Engine
    spec = presets.v2(64, 1024)
    eng = Engine(spec, device=0)
    echo = torch.from_numpy(synth.echo_numpy(spec, 3, seed=4100)).to("cuda:0")
    yield eng, spec, echo
    eng.close()


def _records_by_hand(eng, spec, echo, truth, Ts, cfar, fill):
    """What score.sweep returns, step by step: PC + MTD once, then per T fill(rdm, flag, cfar) and the
    scoring of the flags where they are."""
    import dataclasses
    import torch
    from rsp import score
    B, V, R = echo.shape[0], spec.V, spec.R_out
    rdm = torch.empty((B, V, R), dtype=torch.float32, device=echo.device)
    flag = torch.empty((B, V, R), dtype=torch.uint8, device=echo.device)
    eng.run_dev(echo, rdm=rdm)
    params = score.score_params(v_lim=V, r_lim=R)
    sc = score.Scorer(engine=eng)
    out = []
    for T in Ts:
        fill(rdm, flag, dataclasses.replace(cfar, TR=float(T), TV=float(T)))
        rec = sc.score_dev(flag, rdm, truth, params)
        out.append(dict(T=T, **score.summary(rec, truth, V, R, params, lib=eng.lib)))
    return out


def test_score_sweeps(chain):
    """sweep(detector=...) returns the records of detect_dev's flags scored by hand; sweep without a
    detector returns what the Engine.cfar_dev path gives, as before."""
    from rsp import oscfar, presets, score
    eng, spec, echo = chain
    cfar = presets.default_cfar(spec)
    truth = np.array([[20, 300, 1], [20, 700, 1], [40, 500, 0]], np.int32)
    Ts = (3, 5)
    os_ = oscfar.OsCfar(engine=eng)
    det = oscfar.detector(os_, (7, 7), (True, True))
    got = score.sweep(eng, echo, truth, Ts, cfar, detector=det)
    want = _records_by_hand(eng, spec, echo, truth, Ts, cfar,
                            lambda rdm, flag, c: os_.detect_dev(rdm, c, (7, 7), (True, True), flag=flag))
    np.testing.assert_equal(got, want)
    plain = score.sweep(eng, echo, truth, Ts, cfar)
    want_plain = _records_by_hand(eng, spec, echo, truth, Ts, cfar, lambda rdm, flag, c: eng.cfar_dev(rdm, flag, cfar=c))
    np.testing.assert_equal(plain, want_plain)
    assert [o["fa"].tolist() for o in got] != [o["fa"].tolist() for o in plain]
    assert sum(float(np.nansum(o["fa"])) for o in got) > 0
