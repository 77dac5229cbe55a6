"""tests/mtd_ref.py held to the oracle, and the conditions its scenes must meet -- without a GPU.

mtd_ref is what tests/test_gpu_mtd_instances.py compares the MTD kernels with, so it is pinned
here three ways: to the oracle's own MTD functions (1e-12 relative: both are fp64 FFTs of the same
numbers, eps * log2(V) ~ 1e-15), to a direct O(V^2) DFT sum at small V, and, for the MTI form, to
the oracle's MTI followed by the plain form.  The scenes are checked at every (pin, V) of the
sweep, and every CFAR run of the sweep is run on the oracle alone: its near-threshold mask may
hold at most 0.1 % of the cells and it must see at least one Doppler hit.  A seed or threshold
that fails is changed here (Case.seed_off), not on the GPU.
"""
import functools

import numpy as np
import pytest

import mtd_ref as mr
import prefilter_ref
import rsp_ref as ref
from _util import NEAR_TOL, oracle_flags_c

MASK_CAP = 1e-3


def _rows(pin, R, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((pin, R)) + 1j * rng.standard_normal((pin, R))


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("P", [16, 83, 96, 257])
@pytest.mark.parametrize("div", [150, 20])
def test_matches_process_mtd_and_0v_pressing(P, div):
    pc = _rows(P, 7)
    w = ref.kaiser(P, 8.0)
    want = ref.fun_0v_pressing(ref.fun_Process_MTD(pc, window=w), div)
    got = mr.mtd_ref(pc, w, P, 1, mr.zero_band(P, zero_v_div=div))
    assert _rel(got, want) < 1e-12
    assert (got == 0).all(axis=1).sum() == (want == 0).all(axis=1).sum() > 0


@pytest.mark.parametrize("pin,V,m0", [(12, 16, 1), (100, 128, 2), (300, 512, 0), (64, 64, 3)])
def test_matches_dmx_mtd_pair(pin, V, m0):
    pc = np.stack([_rows(pin, 5, 1), _rows(pin, 5, 2)])
    s_want, d_want = ref.dmx_mtd_pair(pc[0], pc[1], V, m0)
    s, d = mr.mtd_ref(pc, ref.hamming(pin), V, 0, mr.zero_band(V, zero_ends=m0 + 1), beams=2)
    assert _rel(s, s_want) < 1e-12 and _rel(d, d_want) < 1e-12
    assert ((s == 0) == (s_want == 0)).all()
    left, right = mr.beam_magnitudes(pc, ref.hamming(pin), V, 0)
    assert _rel(right - left, d_want) < 1e-12


DFT_SHAPES = [(2, 2), (5, 5), (16, 16), (17, 17), (31, 31), (33, 64), (48, 48), (20, 63), (64, 64)]


@pytest.mark.parametrize("pin,V,lag", [(pin, V, lag) for pin, V in DFT_SHAPES for lag in (0, 1, 3) if lag < pin])
@pytest.mark.parametrize("shift", [0, 1])
def test_matches_direct_dft(pin, V, shift, lag):
    pc = _rows(pin, 3)
    w = ref.hamming(pin)
    x = pc * w[:, None]
    if lag:
        x = np.zeros_like(pc)
        for p in range(pin - lag):
            x[p] = (pc[p + lag] - pc[p]) * w[p]
    want = np.zeros((V, 3))
    for k in range(V):
        acc = np.zeros(3, complex)
        for p in range(pin):
            acc += x[p] * np.exp(-2j * np.pi * k * p / V)
        want[(k + V // 2) % V if shift else k] = np.abs(acc)
    got = mr.mtd_ref(pc, w, V, shift, np.zeros(V, bool), mti_lag=lag)
    assert _rel(got, want) < 1e-12


@pytest.mark.parametrize("pin,V,lag", [(64, 64, 30), (64, 64, 1), (64, 64, 63), (100, 128, 9), (83, 83, 9)])
def test_mti_form_is_the_oracles_mti_then_the_plain_form(pin, V, lag):
    pc = _rows(pin, 4)
    w = ref.kaiser(pin, 8.0)
    zb = mr.zero_band(V, zero_v_div=150)
    want = mr.mtd_ref(prefilter_ref.fun_Process_MTI(pc, lag), w, V, 1, zb)
    assert _rel(mr.mtd_ref(pc, w, V, 1, zb, mti_lag=lag), want) < 1e-12


def test_mti_null_row_is_ill_conditioned_in_any_fp32_transform():
    """Why the GPU sweep measures an MTI case's rows against the median row where a row is smaller:
    at lag 1 the DC row of the noise CPI is the MTI's null, and the same transform in complex64 on
    the CPU (fp32 difference, fp32 window, torch's fp32 FFT) is 1.3e-5 of that row's own norm off
    (asserted: over 3e-6, ten times any row without an MTI) while within 1e-6 of the median row's."""
    import torch
    case = next(c for c in mr.CASES if c.id == "f-p768-lag1")
    x = mr.cpis(case)[0][0]
    want = mr.mtd_ref(x.astype(np.complex128), case.w(), case.V, case.shift, case.band(), case.lag)
    t = torch.from_numpy(x)
    y = torch.zeros_like(t)
    y[:case.pin - 1] = t[1:] - t[:-1]
    got = torch.fft.fft(y * torch.from_numpy(case.w().astype(np.float32))[:, None], dim=0).abs().numpy()
    assert not case.shift and not case.band().any()
    rn = np.linalg.norm(want, axis=1)
    err = np.linalg.norm(got - want, axis=1)
    assert rn[0] < 0.01 * np.median(rn)
    print("MTI null row in complex64: %.2e of its own norm, %.2e of the median row's" % (err[0] / rn[0], err[0] / np.median(rn)))
    assert err[0] / rn[0] > 3e-6 and (err / np.maximum(rn, np.median(rn))).max() < 1e-6


def test_the_table_is_what_the_issue_lists():
    ids = [c.id for c in mr.CASES]
    assert len(set(ids)) == len(ids)
    one = {c.pin for c in mr.CASES if c.id.startswith("a-")}
    assert one == {16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048}
    assert {(c.pin, c.V) for c in mr.CASES if c.id.startswith("c-")} == {
        (33, 64), (100, 128), (257, 512), (1000, 1024), (1025, 2048), (1536, 2048)}
    assert {(c.pin, c.V) for c in mr.CASES if c.beams == 2} == {(512, 512), (300, 512), (1024, 1024), (1536, 2048)}
    assert {c.pin for c in mr.CASES if c.id.startswith("e-")} == {2, 17, 31, 33, 63, 65, 127, 129, 255, 257, 511, 513, 1023}
    assert {(c.pin, c.lag) for c in mr.CASES if c.lag} == {(P, lag) for P in (32, 256, 768, 2048, 129)
                                                           for lag in (1, 9, P - 1)}
    # both branches of the tile remap (32 and 64 tiles per row) on every instance with W < 32
    remap = {}
    for c in mr.CASES:
        if "-x" in c.id:
            remap.setdefault((c.V, c.beams), set()).add(int(c.id.split("-x")[1].split("-")[0]))
    want = {(V, 1): {32, 64} for V in (256, 384, 512, 768, 1024, 1536, 2048)}
    want.update({(V, 2): {32, 64} for V in (512, 1024, 2048)})
    assert remap == want
    # every rotated value meets small, large and 3 * 2^k lengths
    for field, values in (("window", (0, 1, 2)), ("shift", (0, 1))):
        for v in values:
            Vs = {c.V for c in mr.CASES if getattr(c, field) == v}
            assert min(Vs) <= 64 and max(Vs) >= 1024 and any(x % 3 == 0 and x & (x - 1) for x in Vs), (field, v)
    for pick in (lambda c: c.zdiv, lambda c: c.zends, lambda c: not (c.zdiv or c.zends)):
        Vs = {c.V for c in mr.CASES if pick(c)}
        assert min(Vs) <= 64 and max(Vs) >= 1024 and any(x % 3 == 0 for x in Vs)


@functools.lru_cache(maxsize=None)
def _case_planes(case):
    """mtd_ref of the case's three CPIs (the sum plane on two beams), from the complex64 values."""
    x, rows, pa = mr.cpis(case)
    zb = case.band()
    planes = []
    for b in range(3):
        out = mr.mtd_ref(x[b].astype(np.complex128), case.w(), case.V, case.shift, zb, case.lag, case.beams)
        planes.append(out[0] if case.beams == 2 else out)
    return x, rows, pa, zb, planes


@pytest.mark.parametrize("case", mr.CASES, ids=lambda c: c.id)
def test_scenes(case):
    x, rows, (p, a), zb, planes = _case_planes(case)
    pin, V, R = case.pin, case.V, case.R
    assert x.dtype == np.complex64 and x.shape == ((3, pin, R) if case.beams == 1 else (3, 2, pin, R))
    assert 0 < zb.sum() < V // 2 or not (case.zdiv or case.zends)
    # noise: no row outside the band is 0
    assert not (planes[0][~zb] == 0).any() and not planes[0][zb].any()
    # tones: the argmax is the declared row, or that row is in the zero band
    assert rows.shape == (R,) and rows.min() >= 0 and rows.max() < V
    arg = planes[1].argmax(axis=0)
    ok = mr.peaked_columns(planes[1], rows, zb)
    if not case.lag:
        assert ((arg == rows) | zb[rows]).all()
        assert (ok | zb[rows]).all(), "a tone's peak stands less than PEAK_MARGIN over its neighbours"
        edge = [0, 1, V // 2, V - 1] if V > 2 else [0, 1]
        assert set((b + (V // 2 if case.shift else 0)) % V for b in edge) <= set(rows.tolist())
    elif case.lag and pin - case.lag >= 8:
        assert (arg[ok] == rows[ok]).all() and ok.sum() >= R // 2      # (an MTI nulls the tones near k lag = n V)
    # impulses: one pulse per column, the edges among them; flat at |a| w[p] without an MTI
    assert set(min(q, pin - 1) for q in (0, 1, case.G - 1, case.G, pin - 1)) <= set(p.tolist())
    xi = x[2] if case.beams == 1 else x[2][0]
    assert (np.count_nonzero(xi, axis=0) == 1).all() and (xi[p, np.arange(R)] != 0).all()
    assert (np.abs(a) >= 0.49).all() and (np.abs(a) <= 2.01).all()
    if case.beams == 1 and not case.lag:
        want = np.abs(a) * case.w()[p]
        assert np.max(np.abs(planes[2][~zb] - want[None, :]) / want[None, :]) < 1e-12
        assert not planes[2][zb].any()
    if case.lag:
        assert {case.pin - case.lag - 1, case.pin - case.lag} <= set(p.tolist())


CFAR_RUNS = [(c, name, win) for c in mr.CASES for name, win in mr.cfar_windows(c)]


@pytest.mark.parametrize("case,name,win", CFAR_RUNS, ids=lambda v: getattr(v, "id", v if isinstance(v, str) else ""))
def test_cfar_conditions(case, name, win):
    from test_gpu_cfar_dispatch import cfar_obj
    noise_plane = _case_planes(case)[4][0]
    cf = cfar_obj(win, mr.CFAR_T, 0, case.cfar_zdiv, [], case.methods)
    flag, flagV, amb = oracle_flags_c(noise_plane[None], cf, NEAR_TOL)
    assert amb.sum() <= MASK_CAP * amb.size, (case.id, name, int(amb.sum()), amb.size)
    assert flagV.sum() >= 1, (case.id, name)


def test_every_case_but_the_flat_ones_has_a_cfar_run():
    without = {c.id for c in mr.CASES if not mr.cfar_windows(c)}
    assert without == {"e-p2"} | {c.id for c in mr.CASES if c.lag and c.lag == c.pin - 1}
    assert {c.id for c in mr.CASES if [n for n, _ in mr.cfar_windows(c)] == ["w32"]} == {"a-p16", "e-p17"}
