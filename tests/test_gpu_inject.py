"""GPU parity of the target injection (rsp_scr_dev / rsp_inject_dev, csrc/rsp_inject.hip) with
the fp64 restatement of fun_SCR.m / fun_add_clutter.m (tests/scr_ref.py).

Bar: max|gpu - ref| / max|ref| <= 1e-6, the pre-filters' bar: the sums are fp64, the gain is
rounded to fp32 once, the product and the add are fp32 (a numpy emulation of that arithmetic
gives about 1e-7).  As written (complex squares, principal root) the root flips sign across the
negative real axis, so the inputs must keep every |arg g| <= pi - 1e-6; that is asserted on the
reference before the GPU is compared (the margins of the seeds below are 1e-4 rad or more).

Shapes: A the legacy row (odd pitch: 8-byte accesses), B one small segment, C segment
boundaries off every vector edge, D a row that just fills the registers, with gaps between the
segments, E the second-read path, F the second-read path with 8-byte accesses.
"""
import functools
import math

import numpy as np
import pytest

import scr_ref
import score_ref as sr

pytestmark = pytest.mark.gpu

BAR = 1e-6
SCR_DB = (-5.0, 0.0, 10.0)
SHAPES = {   # label: P, R, segments (start, length), seg_db, seed
    "A": (48, 1031, ((0, 82), (82, 242), (324, 707)), (10.0, 0.0, 0.0), 0),
    "B": (16, 64, ((3, 50),), (0.0,), 1),
    "C": (40, 1030, ((0, 81), (81, 243), (324, 706)), (10.0, 0.0, 0.0), 2),
    "D": (8, 4096, ((5, 1000), (1030, 2001), (3100, 990)), (10.0, 0.0, -3.0), 3),
    "E": (4, 16384, ((0, 4001), (4001, 8000), (12003, 4381)), (0.0, 5.0, 0.0), 4),
    "F": (4, 2051, ((1, 1000), (1001, 1050)), (0.0, 3.0), 5),
}


@pytest.fixture(scope="module")
def inj():
    import torch
    assert torch.cuda.is_available()
    from rsp.inject import Injector
    i = Injector(0)
    yield i
    i.close()


def _noise(rng, shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def _inputs(label, batch=3):
    """default_rng(seed) unit complex noise as the clutter; a chirp per segment as the target,
    its amplitude and phase different in every row and CPI, over a little noise everywhere."""
    P, R, segs, db, seed = SHAPES[label]
    rng = np.random.default_rng(seed)
    clutter = _noise(rng, (batch, P, R))
    simu = 0.05 * _noise(rng, (batch, P, R)).astype(np.complex128)
    m = np.arange(P)
    for b in range(batch):
        for a, n in segs:
            k = np.arange(n)
            w = np.exp(1j * np.pi * 0.4 * k * k / n)
            row = (0.5 + b) * (1.0 + 0.2 * np.sin(m)) * np.exp(1j * 0.37 * (b + 1) * m)
            simu[b, :, a:a + n] += np.outer(row, w)
    simu = simu.astype(np.complex64)
    for x in (clutter, simu):
        x.setflags(write=False)
    return simu, clutter


@functools.lru_cache(maxsize=None)
def _ref(label, power):
    P, R, segs, db, _ = SHAPES[label]
    simu, clutter = _inputs(label)
    out, gs = scr_ref.inject(simu, clutter, SCR_DB, segs, db, power)
    out.setflags(write=False)
    return out, gs


def _run(inj, *a, **kw):
    import torch
    out = inj.scr_dev(*a, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _err(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def _outside(R, segs):
    mask = np.ones(R, bool)
    for a, n in segs:
        mask[a:a + n] = False
    return mask


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------ 1. parity, both modes, every path
@pytest.mark.parametrize("power", [scr_ref.ABS2, scr_ref.AS_WRITTEN])
@pytest.mark.parametrize("label", sorted(SHAPES))
def test_scr_dev_matches_restatement(inj, label, power):
    P, R, segs, db, _ = SHAPES[label]
    simu, clutter = _inputs(label)
    want, gs = _ref(label, power)
    if power == scr_ref.AS_WRITTEN:
        margin = scr_ref.arg_margin(gs)
        print("%s: arg margin %.3g rad" % (label, margin))
        assert margin >= 1e-6                      # a condition on the inputs, not a tolerance
    got = _run(inj, simu, clutter, SCR_DB, segs, seg_db=db, power=power)
    e = _err(got, want)
    print("%s power %d: max|d|/max|ref| = %.3g" % (label, power, e))
    assert e <= BAR
    out = _outside(R, segs)
    if out.any():                                   # fun_SCR leaves these columns alone
        np.testing.assert_array_equal(_bits(got[:, :, out]), _bits((simu + clutter)[:, :, out]))


# ------------------------------------------------------------------ 2. add_clutter, clutter pitch and batch
def test_add_clutter_off_and_on(inj):
    P, R, segs, db, _ = SHAPES["C"]
    simu, clutter = _inputs("C")
    for power in (scr_ref.ABS2, scr_ref.AS_WRITTEN):
        y0 = _run(inj, simu, clutter, SCR_DB, segs, seg_db=db, power=power, add_clutter=False)
        y1 = _run(inj, simu, clutter, SCR_DB, segs, seg_db=db, power=power, add_clutter=True)
        want0, _ = scr_ref.inject(simu, clutter, SCR_DB, segs, db, power, add_clutter=False)
        assert _err(y0, want0) <= BAR
        np.testing.assert_array_equal(_bits(y1), _bits(y0 + clutter))   # one fp32 add of the same scaled target


@pytest.mark.parametrize("label,pad", [("C", 6), ("C", 5), ("A", 3), ("E", 2)])
def test_clutter_wider_than_the_target(inj, label, pad):
    """fun_add_clutter's echo(i, 1:point_prt): the clutter rows are `pad` columns longer."""
    import torch
    P, R, segs, db, _ = SHAPES[label]
    simu, clutter = _inputs(label)
    wide = np.full((3, P, R + pad), 1e6 + 1e6j, np.complex64)      # a read past column R would show
    wide[:, :, :R] = clutter
    d_wide = torch.from_numpy(wide).to(inj.device)
    want, _ = _ref(label, scr_ref.ABS2)
    got = _run(inj, simu, d_wide[:, :, :R], SCR_DB, segs, seg_db=db)
    assert _err(got, want) <= BAR
    if (R + pad) % 2 == 0 and R % 2 == 0:           # the same access width: the same bits
        np.testing.assert_array_equal(_bits(got), _bits(_run(inj, simu, clutter, SCR_DB, segs, seg_db=db)))


def test_clutter_batch_cycles(inj):
    P, R, segs, db, _ = SHAPES["C"]
    simu3, clutter = _inputs("C")
    simu = np.concatenate([simu3, simu3[:2] * np.complex64(1.5 - 0.5j)])
    scr = (-5.0, 0.0, 10.0, 3.0, -12.0)
    want, _ = scr_ref.inject(simu, clutter[:2], scr, segs, db, scr_ref.ABS2)      # CPI b uses clutter b % 2
    got = _run(inj, simu, clutter[:2], scr, segs, seg_db=db)
    assert got.shape == (5, P, R) and _err(got, want) <= BAR
    assert _err(got[4], want[4]) <= BAR and _err(got[3], want[3]) <= BAR


# ------------------------------------------------------------------ 3. exact properties
@pytest.mark.parametrize("label", ["B", "D", "F"])
def test_zero_clutter_segment_and_zero_target_row(inj, label):
    P, R, segs, db, _ = SHAPES[label]
    simu, clutter = (x.copy() for x in _inputs(label))
    a, n = segs[-1]
    clutter[1, 2, a:a + n] = 0            # an all-zero clutter segment in one row: gain 0
    a0, n0 = segs[0]
    simu[2, 0, a0:a0 + n0] = 0            # an all-zero target row 1 in a segment of CPI 2: P_s = eps
    for power in (scr_ref.ABS2, scr_ref.AS_WRITTEN):
        got = _run(inj, simu, clutter, SCR_DB, segs, seg_db=db, power=power)
        np.testing.assert_array_equal(_bits(got[1, 2, a:a + n]), _bits(clutter[1, 2, a:a + n]))
        assert np.isfinite(got.view(np.float32)).all()
        assert np.abs(got[2, 1:, a0:a0 + n0]).max() > 1e3       # the rows below are scaled by sqrt(P_echo k / eps)
        np.testing.assert_array_equal(_bits(got[2, 0, a0:a0 + n0]), _bits(clutter[2, 0, a0:a0 + n0]))
        out = _outside(R, segs)
        np.testing.assert_array_equal(_bits(got[:, :, out]), _bits((simu + clutter)[:, :, out]))
        # every other CPI is untouched by the two edits
        want, _ = _ref(label, power)
        assert _err(got[0], want[0]) <= BAR


# ------------------------------------------------------------------ 4. / 5. the point-target form
def _plan(name):
    """Per-CPI different delays and velocities, one target cut by its segment's end, one
    segment without a target (delay -1)."""
    from rsp import inject, presets
    if name == "legacy":
        spec = presets.legacy(48)
        Rg, Vg = [320.0, 1200.0, 4100.0], [-5.7, 12.0, -20.0]      # 4100 m: segment 3 only, cut by the row's end
    else:
        spec = presets.v2(64, 1024)
        Rg, Vg = [320.0, 3900.0, 200.0, 1300.0], [5.0, -8.0, 12.0, -15.0]   # 3900 m: column 650 of segment 2, cut
    plan = inject.target_plan(spec, Rg, Vg, seg_db=[10.0, 0.0, 0.0])
    assert (plan.delay[:, :3] == -1).any() and (plan.delay[:, :3] >= 0).any()
    cut = [(b, s) for b in range(plan.batch) for s, (a, n) in enumerate(plan.segments)
           if plan.delay[b, s] >= 0 and plan.delay[b, s] + len(plan.wf_host[s]) > n]
    assert cut
    return spec, plan


@pytest.mark.parametrize("power", [scr_ref.ABS2, scr_ref.AS_WRITTEN])
@pytest.mark.parametrize("name", ["legacy", "v2"])
def test_inject_dev_matches_scr_dev_and_restatement(inj, name, power):
    import torch
    spec, plan = _plan(name)
    B, P, R = plan.batch, spec.P, spec.R
    clutter = _noise(np.random.default_rng(40 + B), (B, P, R))
    scr = np.array([-5.0, 0.0, 10.0, 4.0][:B])
    simu = scr_ref.echo_simu(P, R, plan.segments, plan.wf_host, plan.delay, plan.dphi)
    want, gs = scr_ref.inject(simu, clutter, scr, plan.segments, plan.seg_db, power)
    if power == scr_ref.AS_WRITTEN:
        # segments without a target have P_s = eps: a positive real, g's argument is the clutter's
        assert scr_ref.arg_margin(gs) >= 1e-6
    got = inj.inject_dev(clutter, plan, scr, power=power)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    e = _err(got, want)
    print("%s power %d: inject_dev vs restatement %.3g" % (name, power, e))
    assert e <= BAR
    mat = _run(inj, simu.astype(np.complex64), clutter, scr, plan.segments, seg_db=plan.seg_db, power=power)
    e2 = _err(got, mat)
    print("%s power %d: inject_dev vs scr_dev on the materialised target %.3g" % (name, power, e2))
    assert e2 <= BAR
    # where there is no target the echo is the clutter
    np.testing.assert_array_equal(got[simu == 0], clutter[simu == 0])


@pytest.mark.parametrize("name", ["legacy", "v2"])
def test_achieved_scr(inj, name):
    """ABS2 without the clutter: sum|out|^2 / sum|clutter|^2 per (row, segment) is the set ratio.
    Bar 1e-6 relative: one fp32 rounding of the gain and one of each product, a few 1e-7 in power."""
    import torch
    spec, plan = _plan(name)
    B, P, R = plan.batch, spec.P, spec.R
    clutter = _noise(np.random.default_rng(50 + B), (B, P, R))
    scr = np.array([-5.0, 0.0, 10.0, 4.0][:B])
    got = inj.inject_dev(clutter, plan, scr, add_clutter=False)
    torch.cuda.synchronize()
    got = got.cpu().numpy().astype(np.complex128)
    c = clutter.astype(np.complex128)
    worst, n_checked = 0.0, 0
    for b in range(B):
        for s, (a, n) in enumerate(plan.segments):
            p_out = np.sum(np.abs(got[b, :, a:a + n]) ** 2, axis=1)
            if plan.delay[b, s] < 0:
                assert (p_out == 0).all()
                continue
            p_c = np.sum(np.abs(c[b, :, a:a + n]) ** 2, axis=1)
            ratio = p_out / p_c / 10.0 ** ((scr[b] + plan.seg_db[s]) / 10.0)
            worst = max(worst, float(np.max(np.abs(ratio - 1.0))))
            n_checked += P
    print("%s: achieved / set SCR - 1, worst of %d (row, segment): %.3g" % (name, n_checked, worst))
    assert n_checked >= 4 * P and worst <= 1e-6


# ------------------------------------------------------------------ 6. in place, determinism, refusals
@pytest.mark.parametrize("label", ["A", "D", "E"])
def test_in_place_and_bit_identical(inj, label):
    import torch
    P, R, segs, db, _ = SHAPES[label]
    simu, clutter = _inputs(label)
    first = _run(inj, simu, clutter, SCR_DB, segs, seg_db=db, power=scr_ref.AS_WRITTEN)
    again = _run(inj, simu, clutter, SCR_DB, segs, seg_db=db, power=scr_ref.AS_WRITTEN)
    np.testing.assert_array_equal(_bits(first), _bits(again))
    d_c = torch.from_numpy(np.array(clutter)).to(inj.device)
    d_s = torch.from_numpy(np.array(simu)).to(inj.device)
    out = inj.scr_dev(d_s, d_c, SCR_DB, segs, seg_db=db, power=scr_ref.AS_WRITTEN, out=d_c)     # on the clutter
    torch.cuda.synchronize()
    assert out is d_c
    np.testing.assert_array_equal(_bits(d_c.cpu().numpy()), _bits(first))
    d_c = torch.from_numpy(np.array(clutter)).to(inj.device)
    inj.scr_dev(d_s, d_c, SCR_DB, segs, seg_db=db, power=scr_ref.AS_WRITTEN, out=d_s)           # on the target
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(d_s.cpu().numpy()), _bits(first))


def test_point_target_in_place_and_bit_identical(inj):
    import torch
    spec, plan = _plan("v2")
    clutter = _noise(np.random.default_rng(60), (plan.batch, spec.P, spec.R))
    d_c = torch.from_numpy(clutter).to(inj.device)
    a = inj.inject_dev(d_c, plan, 3.0).cpu().numpy()
    b = inj.inject_dev(d_c, plan, 3.0).cpu().numpy()
    np.testing.assert_array_equal(_bits(a), _bits(b))
    inj.inject_dev(d_c, plan, 3.0, out=d_c)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(d_c.cpu().numpy()), _bits(a))


def test_refusals(inj):
    import torch
    from rsp import RspError
    P, R, segs, db, _ = SHAPES["B"]
    simu, clutter = _inputs("B")
    d_c = torch.from_numpy(np.array(clutter)).to(inj.device)
    d_s = torch.from_numpy(np.array(simu)).to(inj.device)
    with pytest.raises(RspError, match="overlap"):
        inj.scr_dev(d_s, d_c, 0.0, ((0, 40), (39, 10)))
    with pytest.raises(RspError, match="not inside"):
        inj.scr_dev(d_s, d_c, 0.0, ((30, 35),))
    with pytest.raises(RspError, match="power"):
        inj.scr_dev(d_s, d_c, 0.0, segs, power=7)
    with pytest.raises(RspError, match="d_out == d_clutter"):            # 2 clutter CPIs for 3: not in place
        inj.scr_dev(d_s, d_c[:2], 0.0, segs, out=d_c)
    wide = torch.zeros((3, P, R + 2), dtype=torch.complex64, device=inj.device)
    with pytest.raises(RspError, match="overlaps d_clutter"):            # the output inside a wider clutter
        inj.scr_dev(d_s, wide[:, :, :R], 0.0, segs, out=wide.reshape(-1)[2:3 * P * R + 2].reshape(3, P, R))
    with pytest.raises(RspError, match="overlaps d_simu"):
        big = torch.zeros(3 * P * R + 8, dtype=torch.complex64, device=inj.device)
        inj.scr_dev(big[:3 * P * R].reshape(3, P, R), d_c, 0.0, segs, out=big[8:].reshape(3, P, R))
    with pytest.raises(RspError, match="clutter_batch"):
        inj.scr_dev(d_s[:2], d_c, 0.0, segs)                              # more clutter CPIs than CPIs
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the reference-named wrappers
def test_reference_named_wrappers(inj):
    import torch
    P, R, segs, db, _ = SHAPES["A"]
    simu, clutter = _inputs("A")
    echo = np.concatenate([clutter[0], _noise(np.random.default_rng(9), (P, 9))], axis=1)    # a wider recorded echo
    stc = inj.fun_SCR(P, simu[0], echo, 7.0)
    both = inj.fun_add_clutter(stc, echo)
    torch.cuda.synchronize()
    want, gs = scr_ref.fun_SCR(simu[0], echo, 7.0)                       # the legacy segments, +10/0/0, as written
    assert scr_ref.arg_margin(gs[None]) >= 1e-6
    assert _err(stc.cpu().numpy(), want) <= BAR
    assert _err(both.cpu().numpy(), scr_ref.fun_add_clutter(want, echo)) <= BAR
    np.testing.assert_array_equal(_bits(both.cpu().numpy()), _bits(stc.cpu().numpy() + clutter[0]))
    abs2 = inj.fun_SCR(P, simu[0], echo, 7.0, power=scr_ref.ABS2).cpu().numpy()
    assert _err(abs2, scr_ref.fun_SCR(simu[0], echo, 7.0, power=scr_ref.ABS2)[0]) <= BAR
    assert _err(abs2, want) > 0.1                                          # the two modes really differ


# ------------------------------------------------------------------ 7. end to end: clutter -> injection -> chain -> CFAR -> score
def test_scr_sweep_end_to_end():
    import torch
    from rsp import inject, presets, score
    from rsp.engine import Engine
    spec = presets.v2(64, 1024)
    V, R = spec.V, spec.R_out
    seg = 1                                                   # the 200-sample matched filter's segment
    plan = inject.target_plan(spec, [500.0, 900.0, 1300.0, 1700.0], [5.0, -8.0, 12.0, -15.0])
    truth = plan.truth_cells(spec, seg)
    assert (truth[:, 2] == 1).all() and len(set(truth[:, 0])) == 4 and len(set(truth[:, 1])) == 4
    clutter = torch.from_numpy(_noise(np.random.default_rng(7100), (4, spec.P, spec.R))).to("cuda:0")
    seen = []

    def on_step(scr, flag, rdm, rec):
        torch.cuda.synchronize()
        seen.append((scr, flag.cpu().numpy(), rdm.cpu().numpy(), rec.cpu().numpy()))

    scrs = (-30.0, -10.0, 0.0, 20.0)
    with Engine(spec, device=0) as eng:
        out = score.scr_sweep(eng, clutter, plan, scrs, presets.default_cfar(spec), seg=seg, on_step=on_step)
    assert [o["SCR"] for o in out] == list(scrs) == [s[0] for s in seen]
    p = score.score_params(v_lim=V, r_lim=R)
    kw = dict(n_cell=20, v_lim=V, r_lim=R)
    for o, (scr, f, r, rec) in zip(out, seen):
        want_rec = sr.records(f, r, truth, **kw)
        np.testing.assert_array_equal(rec, want_rec)
        want = score.summary(want_rec, truth, V, R, p)
        np.testing.assert_array_equal(o.pop("fa"), want.pop("fa"))
        o.pop("SCR")
        np.testing.assert_equal(o, want)
    # at +20 dB the target stands where the plan says it is
    _, f, r, rec = seen[-1]
    s = spec.segments[seg]
    for b in range(4):
        sub = r[b][:, s.out_start:s.out_start + s.out_len]
        v, c = np.unravel_index(int(np.argmax(sub)), sub.shape)
        assert abs(v - truth[b, 0]) <= 1 and abs(c + s.out_start - truth[b, 1]) <= 1, (b, v, c, truth[b])
        assert rec[b, 1] > 0                                  # n_box: detected inside the truth's box
    assert out[-1]["drate"] == 1.0
