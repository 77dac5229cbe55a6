"""rsp_cmap_dev on the GPU against the fp64 restatement tests/cmap_ref.py, on its designed scene.

  * band amplitudes and the final map at the project's RDM bars (Frobenius-relative and
    max|d|/max|ref| <= 1e-5);
  * flags against the fp64 recursion fed the GPU's own fp32 amplitudes: exact outside the cells
    whose oracle margin |a - T m| / (T m) is under 1e-5, those counted and capped at 0.1 %
    (as test_gpu_cfar_dispatch.py applies it);
  * the shapes of cmap_ref.CASES, the smallest that reach every instance rsp_cmap_plan reports;
  * identity of bytes between one batch and batches of one, interleaved and separate slots, two
    runs, and overlapping CPIs against dense copies;
  * slot < 0, warmup, hold on and off, and the staged chain at the c3 shape.
The references are computed once per case and shared (module cache).
"""
import dataclasses
import functools

import numpy as np
import pytest

import cmap_ref
from _util import MAX_TOL, RDM_TOL, max_rel, rel_err

pytestmark = pytest.mark.gpu

CASES = {c[0]: c for c in cmap_ref.CASES}
IDS = list(CASES)
# identity of bytes: an 8-byte path, a padded 16-byte path, and the pulse split with two beams
IDENT = ["p33v64-k7-r69", "p128-k13-r200-ld208", "p1536v2048-k64-r70-ld72-beams2"]


@functools.lru_cache(maxsize=None)
def _scene(cid):
    return cmap_ref.case_scene(CASES[cid])


def _cmap(case, w=None, hold=True, warmup=cmap_ref.WARMUP, slots=1, T=cmap_ref.T):
    from rsp.cmap import ClutterMap
    cid, P, V, beams, band, R, ld, window, w0, inst = case
    return ClutterMap(P=P, V=V, beams=beams, window=window, window_beta=8.0, band=band, R=R, slots=slots, T=T,
                      w=w0 if w is None else w, warmup=warmup, hold=hold, fftshift=0)


def _padded(case, x):
    """The frames as a device buffer [F, beams, P, ld], NaN in the padding columns."""
    import torch
    cid, P, V, beams, band, R, ld, window, w0, inst = case
    buf = np.full((x.shape[0], beams, P, ld), np.nan + 1j * np.nan, np.complex64)
    buf[..., :R] = x.reshape(x.shape[0], beams, P, R)
    return torch.from_numpy(buf).cuda()


def _update(cm, case, d_pc, frames=None, slot=None):
    """One call over the frames [lo, hi) of a padded buffer; returns numpy (band, flag)."""
    import torch
    lo, hi = frames if frames is not None else (0, d_pc.shape[0])
    band, flag = cm.update_dev(d_pc[lo:hi], slot=slot, batch=hi - lo, ld=case[6])
    torch.cuda.synchronize()
    return band.cpu().numpy(), flag.cpu().numpy()


def _check_flags(flag, band32, w, hold, warmup=cmap_ref.WARMUP, T=cmap_ref.T, **kw):
    """Flags against the fp64 recursion fed the GPU's amplitudes; returns the restatement's flags."""
    want, _, _, margin = cmap_ref.recursion(band32.astype(np.float64), T, w, warmup, hold, **kw)
    near = margin < cmap_ref.NEAR_TOL
    tested = int(np.isfinite(margin).sum())
    diff = flag != want
    print("flags: %d set, %d tested cells, %d near-threshold, %d differ (%d of them near)"
          % (int(want.sum()), tested, int(near.sum()), int(diff.sum()), int((diff & near).sum())))
    assert int((diff & ~near).sum()) == 0
    assert int(near.sum()) <= 1e-3 * tested
    return want


@pytest.mark.parametrize("w", [0.25, 0.125])
@pytest.mark.parametrize("cid", IDS)
def test_sweep_against_fp64(cid, w):
    case = CASES[cid]
    x, cells, a64 = _scene(cid)
    cm = _cmap(case, w=w)
    plan = cm.plan(cmap_ref.F, ld=case[6])
    assert (plan["bins_per_pass"], plan["vec"], plan["split"]) == case[9]
    band, flag = _update(cm, case, _padded(case, x))
    gmap, gage = cm.map.cpu().numpy(), cm.age.cpu().numpy()
    cm.close()
    e_f, e_m = rel_err(band, a64), max_rel(band, a64)
    _, m64, _, _ = cmap_ref.recursion(a64, cmap_ref.T, w, cmap_ref.WARMUP, True)
    m_f, m_m = rel_err(gmap, m64), max_rel(gmap, m64)
    print("%s w=%g: band rel %.3g max %.3g; map rel %.3g max %.3g" % (cid, w, e_f, e_m, m_f, m_m))
    assert np.isfinite(band).all() and np.isfinite(gmap).all()
    assert e_f <= RDM_TOL and e_m <= MAX_TOL
    assert m_f <= RDM_TOL and m_m <= MAX_TOL
    assert gage.tolist() == [cmap_ref.F]
    want = _check_flags(flag, band, w, True)
    for k, col in cells:
        assert flag[cmap_ref.TONE_FROM:, k, col].all()
    assert int(want[:cmap_ref.WARMUP].sum()) == 0 and int(flag[:cmap_ref.WARMUP].sum()) == 0


def test_sweep_visits_every_instance():
    """Fails when the table leaves an instance the plan can report unvisited (the sweep asserts
    that each case takes the instance the table names)."""
    seen = set()
    for case in cmap_ref.CASES:
        cm = _cmap(case)
        plan = cm.plan(cmap_ref.F, ld=case[6])
        cm.close()
        seen.add((plan["bins_per_pass"], plan["vec"], plan["split"]))
    assert seen == {(kb, vec, split) for kb in (4, 16) for vec in (1, 2) for split in (1, 4)}


@pytest.mark.parametrize("cid", IDENT)
def test_one_batch_equals_batches_of_one_and_a_second_run(cid):
    case = CASES[cid]
    x, _, _ = _scene(cid)
    d_pc = _padded(case, x)
    runs = []
    for split_batches in (False, True, False):
        cm = _cmap(case)
        if split_batches:
            parts = [_update(cm, case, d_pc, (f, f + 1)) for f in range(cmap_ref.F)]
            band, flag = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        else:
            band, flag = _update(cm, case, d_pc)
        runs.append((band, flag, cm.map.cpu().numpy(), cm.age.cpu().numpy()))
        cm.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.tobytes() == b.tobytes()
    # an uneven split, the state carried by the object
    cm = _cmap(case)
    parts = [_update(cm, case, d_pc, fr) for fr in ((0, 5), (5, 6), (6, cmap_ref.F))]
    assert np.concatenate([p[1] for p in parts]).tobytes() == runs[0][1].tobytes()
    assert cm.map.cpu().numpy().tobytes() == runs[0][2].tobytes()
    cm.close()


@pytest.mark.parametrize("cid", IDENT)
def test_interleaved_slots_equal_the_slots_run_apart(cid):
    import torch
    case = CASES[cid]
    x, _, _ = _scene(cid)
    d_a = _padded(case, x)
    d_b = _padded(case, np.ascontiguousarray(x[::-1]) * np.complex64(0.5))     # another history for slot 1
    apart = []
    for d in (d_a, d_b):
        cm = _cmap(case)
        band, flag = _update(cm, case, d)
        apart.append((band, flag, cm.map.cpu().numpy()[0], int(cm.age[0].item())))
        cm.close()
    both = torch.stack([d_a, d_b], dim=1).reshape((2 * cmap_ref.F,) + tuple(d_a.shape[1:])).contiguous()
    cm = _cmap(case, slots=2)
    band, flag = _update(cm, case, both, slot=[0, 1] * cmap_ref.F)
    gmap, gage = cm.map.cpu().numpy(), cm.age.cpu().numpy()
    cm.close()
    for s in (0, 1):
        assert band[s::2].tobytes() == apart[s][0].tobytes()
        assert flag[s::2].tobytes() == apart[s][1].tobytes()
        assert gmap[s].tobytes() == apart[s][2].tobytes() and gage[s] == apart[s][3] == cmap_ref.F
    assert apart[0][1].sum() > 0


@pytest.mark.parametrize("P,R,ld,step,band", [(33, 69, 69, 5, (-3, 3)), (128, 200, 208, 16, (-7, 5)),
                                              (332, 66, 66, 83, (-1, 1))])
def test_overlapping_cpis_equal_dense_copies(P, R, ld, step, band):
    """A window stream: CPI i starts at row i * step of one long block of rows (cpi_stride =
    step * ld < P * ld), against the same CPIs copied out dense."""
    import torch
    from rsp.cmap import ClutterMap
    nf = 10
    rng = np.random.default_rng(cmap_ref.mtd_ref.SEED + P)
    nrows = (nf - 1) * step + P
    rows = (rng.standard_normal((nrows, ld)) + 1j * rng.standard_normal((nrows, ld))).astype(np.complex64)
    rows[:, ::3] += 20.0
    d_rows = torch.from_numpy(rows).cuda()
    dense = np.stack([rows[i * step:i * step + P] for i in range(nf)])
    d_dense = torch.from_numpy(dense).cuda()
    kw = dict(P=P, R=R, band=band, window=1, T=2.0, w=0.25, warmup=2, hold=True, fftshift=0)
    cm = ClutterMap(**kw)
    assert cm.plan(nf, ld=ld, cpi_stride=step * ld)["vec"] == (2 if (step * ld) % 2 == 0 and R % 2 == 0 else 1)
    b1, f1 = cm.update_dev(d_rows, batch=nf, ld=ld, cpi_stride=step * ld)
    cd = ClutterMap(**kw)
    b2, f2 = cd.update_dev(d_dense, batch=nf, ld=ld)
    torch.cuda.synchronize()
    assert b1.cpu().numpy().tobytes() == b2.cpu().numpy().tobytes()
    assert f1.cpu().numpy().tobytes() == f2.cpu().numpy().tobytes()
    assert cm.map.cpu().numpy().tobytes() == cd.map.cpu().numpy().tobytes()
    assert 0 < int(f1.sum().item()) < f1.numel() // 2
    cm.close()
    cd.close()


@pytest.mark.parametrize("cid", ["p33v64-k7-r69", "p332-k3-r66"])
def test_negative_slot_touches_nothing(cid):
    case = CASES[cid]
    x, _, _ = _scene(cid)
    d_pc = _padded(case, x)
    cm = _cmap(case)
    band, flag = _update(cm, case, d_pc)
    ref_state = (cm.map.cpu().numpy(), cm.age.cpu().numpy())
    cm.close()
    skip = [3, 9, 10]                                  # one before the tone, two inside it
    keep = [f for f in range(cmap_ref.F) if f not in skip]
    slot = [-1 if f in skip else 0 for f in range(cmap_ref.F)]
    slot[10] = 7                                       # >= slots: as a negative slot
    cm = _cmap(case)
    band2, flag2 = _update(cm, case, d_pc, slot=slot)
    assert band2.tobytes() == band.tobytes()           # the amplitudes are written all the same
    assert not flag2[skip].any()
    assert cm.age.cpu().numpy().tolist() == [len(keep)]
    want = _check_flags(flag2, band2, case[8], True, slot=slot)
    assert want[keep].sum() > 0
    # the state is that of the kept frames alone
    ck = _cmap(case)
    bk, fk = _update(ck, case, d_pc[keep].contiguous())
    assert fk.tobytes() == flag2[keep].tobytes()
    assert ck.map.cpu().numpy().tobytes() == cm.map.cpu().numpy().tobytes()
    assert ck.map.cpu().numpy().tobytes() != ref_state[0].tobytes()
    cm.close()
    ck.close()


@pytest.mark.parametrize("warmup", [0, 1, 9, 12])
def test_warmup(warmup):
    case = CASES["p128-k13-r200-ld208"]
    x, cells, _ = _scene(case[0])
    cm = _cmap(case, warmup=warmup)
    band, flag = _update(cm, case, _padded(case, x))
    cm.close()
    want = _check_flags(flag, band, case[8], True, warmup=warmup)
    assert not flag[:max(warmup, 1)].any()
    if warmup <= cmap_ref.TONE_FROM:
        for k, col in cells:
            assert flag[cmap_ref.TONE_FROM:, k, col].all()
    if warmup == 12:
        assert not flag.any() and not want.any()


@pytest.mark.parametrize("cid", ["p33v64-k7-r69", "p332-k17-r67", "p1536v2048-k64-r70-ld72-beams2"])
def test_without_hold_the_map_absorbs_the_tone(cid):
    """w = 1/8, hold off: the flagged tone is averaged in, and the restatement says in which
    frame its flag ends; with hold on it stays to the scene's end."""
    case = CASES[cid]
    x, cells, _ = _scene(cid)
    d_pc = _padded(case, x)
    out = {}
    for hold in (False, True):
        cm = _cmap(case, w=0.125, hold=hold)
        band, flag = _update(cm, case, d_pc)
        out[hold] = (flag, cm.map.cpu().numpy())
        cm.close()
        want = _check_flags(flag, band, 0.125, hold)
        for k, col in cells:
            assert flag[:, k, col].tolist() == want[:, k, col].tolist()
            ends = [f for f in range(cmap_ref.TONE_FROM, cmap_ref.F) if not want[f, k, col]]
            if hold:
                assert not ends
            else:
                assert want[cmap_ref.TONE_FROM, k, col] == 1 and ends and ends[0] > cmap_ref.TONE_FROM
                assert not want[ends[0]:, k, col].any()
    k, col = cells[0]
    assert out[False][1][0, k, col] > 2.0 * out[True][1][0, k, col]     # absorbed against held


def test_state_reset_and_load():
    import torch
    case = CASES["p16-k3-r130"]
    x, _, _ = _scene(case[0])
    d_pc = _padded(case, x)
    cm = _cmap(case)
    _update(cm, case, d_pc, (0, 6))
    saved = cm.state()
    b1, f1 = _update(cm, case, d_pc, (6, 12))
    end = cm.map.cpu().numpy()
    cm.load_state(saved)
    assert cm.age.cpu().numpy().tolist() == [6]
    b2, f2 = _update(cm, case, d_pc, (6, 12))
    assert f1.tobytes() == f2.tobytes() and cm.map.cpu().numpy().tobytes() == end.tobytes()
    cm.reset()
    assert cm.age.cpu().numpy().tolist() == [0]
    b3, f3 = _update(cm, case, d_pc, (6, 7))
    assert not f3.any() and cm.map.cpu().numpy()[0].tobytes() == b3[0].tobytes()      # a first frame again
    torch.cuda.synchronize()
    cm.close()


def test_chain_at_c3_merges_band_flags():
    """pc_dev -> mtd_dev with the default CFAR + update_dev on the same rows -> merge_flags: the
    merged plane is the chain's flags outside the band's rows and the band flags inside; and the
    band amplitudes are the rows an MTD without zero band writes there (two fp32 results, each
    within 1e-5 of fp64: 2e-5 between them)."""
    import torch
    from rsp import presets
    from rsp.cmap import ClutterMap, band_of
    from rsp.engine import Engine
    spec = presets.dmx(128, 4096)
    cfar = presets.default_cfar(spec)
    B = 2
    g = torch.Generator(device="cuda").manual_seed(20241020)
    echo = torch.view_as_complex(torch.randn((B, spec.P, spec.R, 2), generator=g, device="cuda")).contiguous()
    echo[1] = echo[1] * 1.5
    eng = Engine(spec)
    pc = torch.empty((B, spec.P, spec.R_out), dtype=torch.complex64, device="cuda")
    rdm = torch.empty((B, spec.V, spec.R_out), dtype=torch.float32, device="cuda")
    flag = torch.empty((B, spec.V, spec.R_out), dtype=torch.uint8, device="cuda")
    eng.pc_dev(echo, pc)
    eng.mtd_dev(pc, rdm=rdm, flag=flag, cfar=cfar)
    assert band_of(spec, cfar) == (-7, 5)
    cm = ClutterMap(spec, cfar=cfar, T=1.2, w=0.25, warmup=1)
    assert cm.K == 13 and cm.plan(B)["bins_per_pass"] == 16 and cm.plan(B)["vec"] == 2 and cm.plan(B)["split"] == 1
    band, bflag = cm.update_dev(pc)
    chain = flag.clone()
    merged = cm.merge_flags(flag, bflag)
    torch.cuda.synchronize()
    rows = cm.rows()
    inside = np.zeros(spec.V, bool)
    inside[rows] = True
    chain, merged, bflag = chain.cpu().numpy(), merged.cpu().numpy(), bflag.cpu().numpy()
    assert not chain[:, inside].any() and chain[:, ~inside].any()          # the chain is blind in the band
    assert (merged[:, ~inside] == chain[:, ~inside]).all()
    assert (merged[:, rows] == bflag).all()
    assert not bflag[0].any() and 0 < int(bflag[1].sum()) < bflag[1].size    # frame 1 at 1.5x over a one-frame map
    _check_flags(bflag, band.cpu().numpy(), 0.25, True, warmup=1, T=1.2)
    # the band is what the MTD writes where it is not zeroed
    open_spec = dataclasses.replace(spec, zero_v_div=0)
    eng2 = Engine(open_spec)
    rdm2 = torch.empty_like(rdm)
    eng2.mtd_dev(pc, rdm=rdm2)
    torch.cuda.synchronize()
    want = rdm2.cpu().numpy()[:, rows].astype(np.float64)
    got = band.cpu().numpy()
    print("band against the open MTD's rows: rel %.3g max %.3g" % (rel_err(got, want), max_rel(got, want)))
    assert rel_err(got, want) <= 2 * RDM_TOL and max_rel(got, want) <= 2 * MAX_TOL
    q_lo, q_hi = band_of(spec)
    assert (rdm.cpu().numpy()[:, cmap_ref.rows(q_lo, q_hi, spec.V, 1)] == 0).all()      # the MTD's own /150 rows
    eng.close()
    eng2.close()
    cm.close()
