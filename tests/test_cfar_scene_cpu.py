"""The designed scenes of tests/cfar_scene.py, for every shape and parameter set of the GPU sweep
(tests/test_gpu_cfar_dispatch.py), without a GPU:

  * the loop-faithful numpy oracle (rsp_ref.fun_CFARflag) and the C oracle (coracle.cfar) give the
    same flags, bit for bit -- the sweep trusts the C one;
  * every feature has the outcome its name claims, worked out from executeCFAR's rules in
    cfar_scene.py, and a spike on a zeroed row changes nothing at all;
  * no feature cell, nor either of its range neighbours, is in the oracle's near-threshold mask --
    except where the feature is an exact tie, which the mask marks by definition (two candidates
    within NEAR_TOL of each other); there the claim itself is the check, here and on the GPU;
  * outside those ties the mask covers at most 0.1 % of the cells;
  * every scene holds the Doppler-edge rows and the range-edge columns, and every kind of feature
    stands in some scene of either table;
  * the dense threshold of every fused case gives some tile of the first chunk more Doppler hits
    than its workgroup has threads (on the designed field; the sweep asserts it on the GPU's RDM).
"""
import numpy as np
import pytest

import cfar_scene as cs
import coracle
import rsp_ref as ref
import test_gpu_cfar_dispatch as sweep
from _util import NEAR_TOL, oracle_cfar_dict

NUMPY_ORACLE_CELLS = 40000     # the numpy oracle loops over hits in Python: the small scenes only


def _sets():
    out = []
    for c in sweep.STANDALONE:
        for T in sweep.THRESHOLDS:
            out.append(pytest.param(sweep.standalone_scenes(c)[0], c, T, c.rflag, id="%s-T%g" % (c.id, T)))
    for c in sweep.FUSED:
        for dense in (False, True):
            T = sweep.fused_T(c, dense)
            out.append(pytest.param(sweep.fused_scenes(c)[0], c, T, 1, id="fused-%s-T%g" % (c.id, T)))
    return out


def _zone(cells, shape):
    z = np.zeros(shape, bool)
    for v, c in cells:
        z[v, max(c - 1, 0):c + 2] = True
    return z


@pytest.mark.parametrize("sc,case,T,rflag", _sets())
def test_scene(sc, case, T, rflag):
    V, R = sc.field.shape
    cf = sweep.cfar_obj(case.win, T, case.M0, case.zdiv, sc.segments, case.methods, rflag)
    d = oracle_cfar_dict(cf)
    segs0 = list(sc.segments) or [(0, R)]
    mtd_zdiv = getattr(case, "mtd_zdiv", 0)
    field = ref.fun_0v_pressing(sc.field, mtd_zdiv) if mtd_zdiv else sc.field   # as the MTD returns it
    flag, flagV, amb = (a[0] for a in coracle.cfar(field, d, segs0, near_tol=NEAR_TOL))
    if V * R <= NUMPY_ORACLE_CELLS:
        nf, nfv, namb = ref.main_cfar_chain(field, d, [(a + 1, b) for a, b in segs0], cf.zero_v_div, near_tol=NEAR_TOL)
        assert (nf == flag).all() and (nfv == flagV).all() and (namb == amb).all()
    # the claims
    for f, (v, c), fv, fl in cs.claimed(sc, rflag):
        assert fv is None or flagV[v, c] == fv, (f.name, v, c, "flagV", fv)
        assert fl is None or flag[v, c] == fl, (f.name, v, c, "flag", fl)
    for f in sc.features:
        if f.erased:
            g, gv = coracle.cfar(sc.without(f) if not mtd_zdiv else ref.fun_0v_pressing(sc.without(f), mtd_zdiv), d, segs0)
            assert (g[0] == flag).all() and (gv[0] == flagV).all(), f.name
    # the mask
    plain = [(v, c) for f in sc.features if not f.tie for v, c, x in f.cells if x > cs.QUIET and f.kind != "zeros"]
    assert not (amb & _zone(plain, amb.shape)).any()
    assert (amb & ~sweep.tie_zone(sc)).sum() <= sweep.MASK_CAP * amb.size
    # what every scene holds
    missing = [n for n in sc.skipped if n.startswith(("doppler:", "seg", "gap"))]
    assert not missing, missing
    if hasattr(case, "dense_T") and T == case.dense_T:
        W, threads, _ = sweep.TILE[case.P]
        per_tile = [int(flagV[:, t:t + W].sum()) for t in range(0, R, W)]
        assert max(per_tile) > threads, (max(per_tile), threads)


def test_every_kind_stands_somewhere():
    want = {"doppler-edge", "range-edge", "range-gap", "word-pair", "word-edge", "reloc", "reloc-tie",
            "reloc-boundary", "run", "zeros"}
    names = {"word16", "word16-mirror", "word4", "word4-mirror", "edge16", "edge16+2", "reloc-moved", "reloc-equal",
             "reloc-plateau", "reloc-boundary", "run", "zeros"}
    for table, scenes in ((sweep.STANDALONE, sweep.standalone_scenes), (sweep.FUSED, sweep.fused_scenes)):
        kinds, seen = set(), set()
        for c in table:
            s = scenes(c)[0]
            kinds |= s.kinds()
            seen |= {f.name for f in s.features}
        if table is sweep.FUSED:   # no room for the full-height block in rows this short: the small one
            kinds = {"zeros" if k == "zeros-small" else k for k in kinds}
            seen = {"zeros" if n == "zeros-small" else n for n in seen}
        assert want <= kinds, want - kinds
        assert names <= seen, names - seen


def test_layouts():
    """The four-segment layout: out of order, one gap, odd boundaries, an edge on a multiple of 16, one
    at 16k + 2, one segment of exactly 2 * (ref + guard) cells."""
    for R, w in ((272, 12), (268, 12), (269, 30), (4112, 12), (272, 1)):
        segs = cs.layout(R, w, 4)
        assert segs != sorted(segs)
        s = sorted(segs)
        assert any(b - a == 2 * w for a, b in s)
        assert sum(1 for (_, b), (a, _) in zip(s, s[1:]) if a > b) == 1
        assert any(a % 16 == 0 for a, _ in s) and any(a % 16 == 2 for a, _ in s)
        assert s[0][0] % 2 == 1 and s[-1][1] == R - 1
        assert all(b - a >= 2 * w for a, b in s)
