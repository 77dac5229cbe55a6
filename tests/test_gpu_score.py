"""GPU parity of the detection scoring (rsp_score_dev, csrc/rsp_score.hip) against the fp64
restatement of main_cfar.m:163-279 (tests/score_ref.py).

Bar: exact.  The record is eight integers per CPI -- flag sums, status bits, the number of
cells equal to a maximum and the first of them -- so every field must be identical to the
restatement's, whatever path (16-byte or byte loads, one or many workgroups per CPI) made it.

The cases the scoring has to tell apart need five valid truths (one per branch of fun_PCF's
if / elseif chain) and an invalid one, which is six; the batches of 5 here therefore come as
two truth sets, A and B, over the same planes.  Between them: a valid interior truth, an
invalid one, a detection box that leaves the matrix low and one that leaves it high, each
of the five fun_PCF branches, a PCF box that holds no flag, a PCF box that is an index error,
and an RDM whose box maximum occurs a second time elsewhere (n_peak == 2).
"""
import numpy as np
import pytest

import score_ref as sr

pytestmark = pytest.mark.gpu

N_CELL = 20


@pytest.fixture(scope="module")
def scorer():
    import torch
    assert torch.cuda.is_available()
    from rsp.score import Scorer
    s = Scorer(0)
    yield s
    s.close()


def _truths(V, R):
    """Two sets of 5 truths {v_idx, r_idx, valid} (0-based) for a V x R matrix, V, R >= 64."""
    vm, rm = V // 2, R // 2
    A = [[vm, rm, 1],          # interior: box inside, last PCF branch; made a repeated maximum below
         [vm, rm, 0],          # not valid
         [vm, 2, 1],           # detection box leaves low (columns); PCF: columns below 1
         [V - 2, rm, 1],       # detection box leaves high (rows); PCF: rows above v_lim
         [10, rm - 30, 1]]     # PCF: rows below 1; its box is emptied of flags below
    B = [[vm + 1, rm + 60, 1], # interior (clear of A[0]'s box), one maximum
         [3, 9, 0],            # not valid, near a corner
         [vm, R - 10, 1],      # PCF: columns above r_lim, detection box inside
         [1, rm, 1],           # detection box leaves low (rows); PCF: rows below 1
         [5, R - 3, 1]]        # box leaves high (columns); PCF clips rows only -> columns are an index error
    return np.array(A, np.int32), np.array(B, np.int32)


def _scene(seed, V, R, density=0.004):
    """5 planes: sparse flags, a positive RDM, a peak with a detection next to every A/B truth."""
    rng = np.random.default_rng(seed)
    fl = (rng.random((5, V, R)) < density).astype(np.uint8)
    rdm = (rng.random((5, V, R)) + 0.25).astype(np.float32)
    A, B = _truths(V, R)
    for b in range(5):
        for k, t in enumerate((A[b], B[b])):
            v, r = min(max(t[0] + 2, 0), V - 1), min(max(t[1] - 3, 0), R - 1)
            fl[b, v, r] = 1
            rdm[b, v, r] = 40.0 + b + 0.5 * k
    # A[0]: the interior truth's box maximum once more, far outside the box and EARLIER in find()
    # order (a smaller column), so the first match is the far one
    v, r = A[0][0] + 2, A[0][1] - 3
    rdm[0, v, r] = 90.0
    rdm[0, V - 1, 1] = 90.0
    # A[4]: no flag in its PCF box (rows 0..30, columns r-20..r+20)
    fl[4, 0:31, A[4][1] - N_CELL:A[4][1] + N_CELL + 1] = 0
    return fl, rdm, A, B


def _kw(V, R):
    return dict(n_cell=N_CELL, v_lim=V, r_lim=R)


def _score(scorer, fl, rdm, truth, V, R, **win):
    import torch
    rec = scorer.score_dev(fl, rdm, truth, scorer.params(**_kw(V, R)), **win)
    torch.cuda.synchronize()
    return rec.cpu().numpy()


def _same(got, want):
    for k, name in enumerate(("n_flags", "n_box", "box_status", "n_pcf", "pcf_status", "n_peak", "peak_v", "peak_r")):
        np.testing.assert_array_equal(got[:, k], want[:, k], err_msg=name)


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("V,R", [(155, 288), (64, 250)])     # the reference's size (16-byte rows) / byte path
def test_records_match_restatement(scorer, V, R, which):
    fl, rdm, A, B = _scene(V * 1000 + R, V, R)
    truth = A if which == "A" else B
    want = sr.records(fl, rdm, truth, **_kw(V, R))
    # the batch holds the cases it was built for
    if which == "A":
        assert want[0, 2] == 0 and want[0, 5] == 2 and (want[0, 6], want[0, 7]) == (V - 1, 1)
        assert list(want[1, 1:]) == [0] * 7 and want[1, 0] > 0
        assert want[2, 2] == 1 and want[2, 4] == 0 and want[2, 3] > 0
        assert want[3, 2] == 2 and want[3, 4] == 0 and want[3, 3] > 0
        assert want[4, 3] == 0 and want[4, 5] == 0 and want[4, 2] == 0
        assert sr.pcf_ranges(A[2][0] + 1, A[2][1] + 1, **_kw(V, R))[2] == 1            # columns clipped low
        assert sr.pcf_ranges(A[3][0] + 1, A[3][1] + 1, **_kw(V, R))[1] == V            # rows clipped high
        assert sr.pcf_ranges(A[4][0] + 1, A[4][1] + 1, **_kw(V, R))[0] == 1            # rows clipped low
    else:
        assert want[0, 2] == 0 and want[0, 5] == 1 and want[0, 3] > 0
        assert sr.pcf_ranges(B[0][0] + 1, B[0][1] + 1, **_kw(V, R)) == (B[0][0] - 19, B[0][0] + 21, B[0][1] - 19, B[0][1] + 21)
        assert sr.pcf_ranges(B[2][0] + 1, B[2][1] + 1, **_kw(V, R))[3] == R            # columns clipped high
        assert want[2, 2] == 0 and want[2, 5] == 1
        assert want[3, 2] == 1 and want[3, 5] == 1
        assert want[4, 2] == 2 and want[4, 4] == 1 and want[4, 3] == 0 and want[4, 5] == 0
    _same(_score(scorer, fl, rdm, truth, V, R), want)


@pytest.mark.parametrize("cols", [(100, 900), (96, 896)])    # an odd column offset (byte loads) / a 16-byte one
def test_window_of_a_larger_plane(scorer, cols):
    rows = (30, 94)
    V, R = rows[1] - rows[0], cols[1] - cols[0]
    # the surroundings are full of flags and large values: a load outside the window would show
    big_f = np.ones((5, 128, 1024), np.uint8)
    big_r = np.full((5, 128, 1024), 1000.0, np.float32)
    fl, rdm, A, B = _scene(71, V, R)
    big_f[:, rows[0]:rows[1], cols[0]:cols[1]] = fl
    big_r[:, rows[0]:rows[1], cols[0]:cols[1]] = rdm
    for truth in (A, B):
        got = _score(scorer, big_f, big_r, truth, V, R, rows=rows, cols=cols)
        _same(got, sr.records(fl, rdm, truth, **_kw(V, R)))


@pytest.mark.parametrize("value", [0, 1])
@pytest.mark.parametrize("V,R", [(155, 288), (64, 250)])
def test_all_zero_and_all_one_planes(scorer, V, R, value):
    fl = np.full((5, V, R), value, np.uint8)
    _, rdm, A, B = _scene(5, V, R)
    want = sr.records(fl, rdm, A, **_kw(V, R))
    assert (want[:, 0] == value * V * R).all()
    _same(_score(scorer, fl, rdm, A, V, R), want)


@pytest.mark.parametrize("V,R", [(155, 288), (64, 250)])
def test_without_rdm(scorer, V, R):
    fl, _, A, B = _scene(9, V, R)
    for truth in (A, B):
        want = sr.records(fl, None, truth, **_kw(V, R))
        assert (want[:, 5:] == 0).all() and want[:, 3].max() > 0
        _same(_score(scorer, fl, None, truth, V, R), want)


@pytest.mark.parametrize("batch,V,R", [(130, 64, 256), (2100, 48, 64)])    # bands of rows per CPI / one workgroup per CPI
def test_many_cpis(scorer, batch, V, R):
    rng = np.random.default_rng(batch)
    fl = (rng.random((batch, V, R)) < 0.01).astype(np.uint8)
    rdm = rng.random((batch, V, R), dtype=np.float32) + 0.25
    truth = np.stack([rng.integers(0, V, batch), rng.integers(0, R, batch), rng.integers(0, 4, batch) > 0],
                     axis=1).astype(np.int32)
    got = _score(scorer, fl, rdm, truth, V, R)
    np.testing.assert_array_equal(got[:, 0], fl.reshape(batch, -1).sum(1))
    pick = np.unique(np.concatenate([np.arange(0, batch, max(1, batch // 24)), [batch - 1]]))
    want = sr.records(fl[pick], rdm[pick], truth[pick], **_kw(V, R))
    assert (want[:, 5] > 0).sum() >= 5 and (want[:, 4] > 0).any() and (want[:, 2] > 0).any()
    _same(got[pick], want)


# ------------------------------------------------------------------ on the real chain
P_C1, R_C1 = 64, 1024     # the c1 shape


@pytest.fixture(scope="module")
def chain():
    import torch
    from rsp import presets, synth
    from rsp.engine import Engine
    spec = presets.v2(P_C1, R_C1)
    eng = Engine(spec, device=0)
    echo = torch.from_numpy(synth.echo_numpy(spec, 3, seed=4100)).to("cuda:0")
    # synth's targets: (delay column, velocity) -> (Doppler row after fftshift, column)
    rp = spec.radar
    cells = [(int(round(2 * v / rp["wavelength"] * spec.P * rp["prt"])) + spec.P // 2, d) for _, d, v in synth._targets(spec)]
    yield eng, spec, echo, cells
    eng.close()


def test_chain_end_to_end(chain, scorer):
    import torch
    from rsp import presets
    eng, spec, echo, cells = chain
    V, R = spec.V, spec.R_out
    rdm = torch.empty((3, V, R), dtype=torch.float32, device="cuda:0")
    flag = torch.empty((3, V, R), dtype=torch.uint8, device="cuda:0")
    eng.run_dev(echo, rdm=rdm, flag=flag, cfar=presets.default_cfar(spec))
    # CPI 0: truth on the second target; CPI 1: on empty noise far from all three; CPI 2: on the first
    truth = np.array([[cells[1][0], cells[1][1], 1], [20, 700, 1], [cells[0][0], cells[0][1], 1]], np.int32)
    got = _score(scorer, flag, rdm, truth, V, R)
    f, r = flag.cpu().numpy(), rdm.cpu().numpy()
    _same(got, sr.records(f, r, truth, **_kw(V, R)))
    assert got[0, 1] > 0 and got[2, 1] > 0 and got[1, 1] == 0
    assert got[0, 5] == 1 and abs(got[0, 6] - truth[0, 0]) <= 3 and abs(got[0, 7] - truth[0, 1]) <= 7


def test_sweep(chain):
    import torch
    from rsp import presets, score
    eng, spec, echo, cells = chain
    V, R = spec.V, spec.R_out
    truth = np.array([[cells[1][0], cells[1][1], 1], [20, 700, 1], [cells[0][0], cells[0][1], 0]], np.int32)
    seen = []

    def on_step(T, flag, rdm, rec):
        torch.cuda.synchronize()
        seen.append((T, flag.cpu().numpy(), rdm, rdm.cpu().numpy()))

    Ts = (4, 5, 7)
    out = score.sweep(eng, echo, truth, Ts, presets.default_cfar(spec), on_step=on_step)
    assert [o["T"] for o in out] == list(Ts) and [s[0] for s in seen] == list(Ts)
    assert all(s[2] is seen[0][2] for s in seen)                 # one RDM tensor for every T
    p = score.score_params(v_lim=V, r_lim=R)
    counts = []
    for o, (T, f, _, r) in zip(out, seen):
        np.testing.assert_array_equal(r, seen[0][3])
        want = score.summary(sr.records(f, r, truth, **_kw(V, R)), truth, V, R, p)
        np.testing.assert_array_equal(o.pop("fa"), want.pop("fa"))
        o.pop("T")
        np.testing.assert_equal(o, want)                         # NaN-aware
        counts.append(int(f.sum()))
    assert min(counts) > 0
    assert out[1]["drate"] == 0.5 and out[1]["n_valid"] == 2


# ------------------------------------------------------------------ the reference-named wrappers
def test_reference_named_wrappers(scorer):
    V, R = 155, 288
    r_axis = 6.0 * np.arange(R)                                              # main_cfar.m:65
    v_axis = (np.linspace(-7706.5, 7706.5, 1536) * 0.0545 / 2)[690:845]      # :66-68
    n = 6
    rng = np.random.default_rng(3)
    fl = (rng.random((n, V, R)) < 0.003).astype(np.float64)                  # MATLAB doubles
    mtd = (rng.random((n, V, R)) + 0.25).astype(np.float32)
    Rt = np.array([900.0, 1200.0, 300.0, 1500.0, 600.0, 1000.0])
    Vt = np.array([10.0, -8.0, 10.0, 1.0, -15.0, 5.0])
    ids = [1, 2, 3, 4, 5, 6]
    for i in range(n):
        vi, ri = sr.nearest_index(v_axis, Vt[i]), sr.nearest_index(r_axis, Rt[i])
        fl[i, vi + 1, ri - 4] = 1
        mtd[i, vi, ri + 2] = 30.0 + i
    fl[4] = 0
    args = (fl, Rt, Vt, r_axis, v_axis, ids)
    assert scorer.fun_drate(*args) == sr.fun_drate(*args) == 3 / 4
    assert scorer.fun_accuracy(*args) == sr.fun_accuracy(*args)
    want = sr.fun_PCF(*args, mtd)
    assert abs(scorer.fun_PCF(*args, mtd) - want) <= 1e-14 and 0 < want < 1
    for i in range(n):
        vi, ri = sr.nearest_index(v_axis, Vt[i]), sr.nearest_index(r_axis, Rt[i])
        assert scorer.fun_frame_fa(fl[i], Rt[i], Vt[i], ri, vi) == sr.fun_frame_fa(fl[i], Rt[i], Vt[i], ri, vi)
    # the two ways the reference stops
    edge_R, edge_V = np.array([6.0 * 286]), np.array([10.0])                 # columns 280..294 of 288
    one = (fl[:1], edge_R, edge_V, r_axis, v_axis, [1])
    for name in ("fun_drate", "fun_accuracy"):
        with pytest.raises(IndexError):
            getattr(sr, name)(*one)
        with pytest.raises(IndexError):
            getattr(scorer, name)(*one)
    with pytest.raises(IndexError):
        sr.fun_frame_fa(fl[0], 900.0, 10.0, 3, 80)
    with pytest.raises(IndexError):
        scorer.fun_frame_fa(fl[0], 900.0, 10.0, 3, 80)
    mtd2 = mtd.copy()
    mtd2[0, 0, 0] = 30.0                                                     # frame 1's maximum a second time
    with pytest.raises(ValueError):
        sr.fun_PCF(*args, mtd2)
    with pytest.raises(ValueError):
        scorer.fun_PCF(*args, mtd2)
