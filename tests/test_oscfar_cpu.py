"""The ordered-statistic CFAR's restatement (tests/oscfar_ref.py) held to itself, to the existing
oracle and to the rule, on the scenes the GPU sweep runs (no GPU needed):

  * the sorted form equals the counting form, flag for flag, on every scene and case;
  * the sorted form (fp32 product) equals the plain fp64 form on every cell whose margin
    |z - T w| / (T w) exceeds 1e-6, and at most 1 % of a scene's cells lie inside that margin;
  * with ref = 1, k = 1, T = 4 (every product exact) the per-side GO and SO forms are the existing
    detector: oracle/rsp_ref.py's fun_CFARflag, bit for bit;
  * every scene carries a detection where a kernel that ignores an edge would lose it;
  * the masking scene's claims follow from the rule alone.
"""
import numpy as np
import pytest

import oscfar_ref as osr
import rsp_ref as ref

ALL_SHAPES = osr.SHAPES + osr.TILE_SHAPES
IDS = [s.name for s in ALL_SHAPES]


def _cases(shape):
    return osr.cases(shape) if shape in osr.SHAPES else [(osr.UNION, shape.ref, 1)]


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=IDS)
def test_sorted_form_equals_counting_form(shape):
    x = osr.scene(shape)
    for form, k, rf in _cases(shape):
        p = shape.params(form, k, rf)
        for b in range(shape.batch):
            a, c = osr.os_cfar(x[b], p), osr.os_cfar_counting(x[b], p)
            for key in ("flag", "flagV", "passR"):
                assert np.array_equal(a[key], c[key]), (form, k, rf, b, key)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=IDS)
def test_fp32_product_equals_fp64_off_the_margin(shape):
    x = osr.scene(shape)
    for form, k, _ in [c for c in _cases(shape) if c[2] == 1]:
        p = shape.params(form, k, 1)
        for b in range(shape.batch):
            cells = inside = 0
            for stage, Z, lo, hi, args, _ in osr.stage_lines(x[b], p):
                got, _ = osr.os_line(Z, lo, hi, *args)
                want, margin = osr.os_line64(Z, lo, hi, *args)
                far = margin[:, lo:hi] > 1e-6
                assert np.array_equal(got[:, lo:hi][far], want[:, lo:hi][far]), (form, k, b, stage)
                cells += far.size
                inside += int((~far).sum())
            assert inside <= 0.01 * cells, "%d of %d cells within 1e-6 of their threshold" % (inside, cells)


@pytest.mark.parametrize("form", [osr.GO, osr.SO])
@pytest.mark.parametrize("rflag", [0, 1])
def test_rank_one_of_one_cell_is_the_existing_detector(form, rflag):
    """ref = 1: the mean of a window is its one cell, which is also its 1st smallest; T = 4 makes
    every product exact in fp32 and fp64."""
    V, R, save, M0 = 64, 130, 2, 2
    segs = osr.cfar_scene.layout(R, 1 + save, 3)
    x = osr.scene(osr.SHAPES[2])[0][:V, :R]
    p = osr.Params(1, save, 1, save, M0, tuple(segs), 0, 4.0, 4.0, form, 1, 1, rflag)
    got = osr.os_cfar(x, p)
    m = p.method
    flag, flagV = ref.fun_CFARflag(x.astype(np.float64), 1, save, 4.0, m, 1, save, 4.0, m, M0, rflag,
                                   segments=[(a + 1, b) for a, b in segs])
    assert flag.sum() > 0 and (rflag == 0 or not np.array_equal(flag, flagV))
    assert np.array_equal(got["flagV"], flagV.astype(np.uint8))
    assert np.array_equal(got["flag"], flag.astype(np.uint8))


@pytest.mark.parametrize("shape", osr.SHAPES, ids=[s.name for s in osr.SHAPES])
def test_scene_audit(shape):
    """Under the restatement every case of the sweep flags the first and the last band row, a
    one-sided-left and a one-sided-right cell of every segment in both stages, a re-localised range
    hit and a Doppler hit that the range test drops."""
    x = osr.scene(shape)
    V, R = shape.V, shape.R
    lo, hi = shape.M0 + 1, V - shape.M0
    wv = wr = shape.ref + shape.save
    rows = np.arange(V)
    for form, k, rf in osr.cases(shape):
        p = shape.params(form, k, rf)
        for b in range(shape.batch):
            r = osr.os_cfar(x[b], p)
            tag = (form, k, rf, b)
            assert r["flag"][lo].any() and r["flag"][hi - 1].any(), tag
            for a, e in shape.segments or [(0, R)]:
                fv = r["flagV"][:, a:e]
                assert fv[(rows >= lo) & (rows - wv < lo)].any(), (tag, a, e, "Doppler one-sided left")
                assert fv[(rows < hi) & (rows + wv >= hi)].any(), (tag, a, e, "Doppler one-sided right")
                if rf:
                    fl = r["flag"][lo:hi]
                    assert fl[:, a:min(a + wr, e)].any(), (tag, a, e, "range one-sided left")
                    assert fl[:, max(e - wr, a):e].any(), (tag, a, e, "range one-sided right")
            if rf:
                assert r["moved"].any(), (tag, "no re-localised hit")
                assert r["dropped"].any(), (tag, "no Doppler hit dropped by the range test")
                assert not np.array_equal(r["flag"], r["flagV"])


def test_zero_block_and_zero_band_are_in_the_sweep():
    """One scene has exact zeros over whole windows (threshold 0: a zero cell passes, also at the
    largest rank of the greatest-of form, which needs every window cell to be zero), one case runs
    with a zero_v_div band."""
    assert any(s.zero_v_div for s in osr.SHAPES)
    found = 0
    for s in osr.SHAPES:
        x = osr.scene(s)[0]
        r = osr.os_cfar(x, s.params(osr.GO, s.ref, 1))
        found += int(((x == 0) & (r["flagV"] == 1) & (r["flag"] == 1)).sum())
    assert found > 0


def test_masking_claims_follow_from_the_rule():
    x, a, b = osr.masking_scene()
    noise = x.copy()
    noise[a] = noise[b] = 0
    assert noise.max() < 5.0
    kw = osr.MASK_PARAMS
    # GO on means: the existing detector's rule, from the oracle
    _, flagV = ref.executeCFAR(x.astype(np.float64), kw["refR"], kw["saveR"], kw["TR"], 0, kw["refV"], kw["saveV"],
                               kw["TV"], 0, kw["M0"], 0)
    assert flagV[a] == 0 and flagV[b] == 0
    p = osr.Params(form=osr.UNION, kV=7, kR=7, **kw)
    r = osr.os_cfar(x, p)
    assert r["flagV"][a] == 1 and r["flagV"][b] == 1
    # and the per-side greatest-of the largest rank is masked as the mean is
    r5 = osr.os_cfar(x, osr.Params(form=osr.GO, kV=5, kR=5, **kw))
    assert r5["flagV"][a] == 0 and r5["flagV"][b] == 0


def test_plan_needs_no_gpu_and_the_shapes_cover_every_tile_width():
    """rsp_os_cfar_plan is host arithmetic (no context, no GPU): the sweep's shapes and the narrow
    planes take every Doppler tile width there is for V <= 4096, and both range stages."""
    import ctypes as C
    from rsp import _capi as capi
    from rsp.oscfar import os_params
    from rsp.presets import Cfar
    lib = capi.load_library()
    seen = set()
    for s in ALL_SHAPES:
        for rf in (0, 1):
            cp = Cfar(refR=s.ref, saveR=s.save, refV=s.ref, saveV=s.save, M0=s.M0, rFlag=rf, zero_v_div=s.zero_v_div,
                      segments=list(s.segments)).to_c()
            op = os_params((1, 1))
            out = capi.rsp_os_plan_t()
            assert lib.rsp_os_cfar_plan(None, s.V, s.R, s.batch, C.byref(cp), C.byref(op), 1, C.byref(out)) == 0
            assert out.v_pitch >= s.V and out.v_pitch % 32 == max(1, 32 >> out.v_tile_log2) % 32
            assert 2 * 4 * (out.v_pitch << out.v_tile_log2) <= 80 * 1024
            seen.add((out.v_tile_log2, out.r_stage))
    assert seen == {(lw, r) for lw in range(1, 7) for r in (capi.RSP_OS_R_NONE, capi.RSP_OS_R_GATHER)}
    op = os_params((0, 1))
    assert lib.rsp_os_cfar_plan(None, 64, 64, 1, C.byref(cp), C.byref(op), 1, C.byref(out)) == capi.RSP_ERR_ARG
    assert b"kV" in lib.rsp_last_error(None)
