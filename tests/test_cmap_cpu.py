"""Clutter map, CPU side: the restatement tests/cmap_ref.py against hand-computed recursions,
band_of against the MTD's own zero band, the designed scene's conditions in fp64, and the C ABI's
declaration, struct layout, plan and refusals (rsp_cmap_dev checks everything it can before it
looks at the context).
"""
import ctypes as C
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

import cmap_ref
import mtd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the recursion by hand
def _cell(values, **kw):
    a = np.asarray(values, np.float64).reshape(-1, 1, 1)
    flag, m, age, _ = cmap_ref.recursion(a, **kw)
    return flag[:, 0, 0].tolist(), float(m[0, 0, 0]), age.tolist()


def test_first_frame_initialises_and_flags_nothing():
    flag, m, age = _cell([7.0], T=0.5, w=0.25, warmup=0, hold=True)
    assert flag == [0] and m == 7.0 and age == [1]       # warmup 0 counts as 1: a >= T m, yet no flag
    flag, m, age = _cell([7.0, 3.0], T=4.0, w=0.25, warmup=1, hold=True)
    assert flag == [0, 0] and m == 7.0 + 0.25 * (3.0 - 7.0) and age == [2]


def test_warmup_edge():
    # a spike of 100 over a map of 1: flagged only once the slot has absorbed `warmup` CPIs
    vals = [1.0, 1.0, 100.0]
    assert _cell(vals, T=4.0, w=0.5, warmup=2, hold=True)[0] == [0, 0, 1]
    flag, m, age = _cell(vals, T=4.0, w=0.5, warmup=3, hold=True)
    assert flag == [0, 0, 0] and m == 1.0 + 0.5 * 99.0 and age == [3]     # unflagged: absorbed, hold or not
    assert _cell(vals + [400.0], T=4.0, w=0.5, warmup=3, hold=True)[0] == [0, 0, 0, 1]   # 400 >= 4 * 50.5


def test_hold_keeps_the_map_and_no_hold_absorbs():
    vals = [2.0, 2.0, 16.0, 16.0, 16.0, 16.0]
    flag, m, _ = _cell(vals, T=4.0, w=0.5, warmup=1, hold=True)
    assert flag == [0, 0, 1, 1, 1, 1] and m == 2.0                        # 16 >= 8, held: the map never moves
    flag, m, _ = _cell(vals, T=4.0, w=0.5, warmup=1, hold=False)
    # m: 2, 2, 9 (16 >= 8 flagged, absorbed), 12.5 (16 < 36), 14.25, 15.125
    assert flag == [0, 0, 1, 0, 0, 0] and m == 15.125
    # the threshold is inclusive
    assert _cell([2.0, 8.0], T=4.0, w=0.5, warmup=1, hold=True)[0] == [0, 1]
    assert _cell([2.0, np.nextafter(8.0, 0.0)], T=4.0, w=0.5, warmup=1, hold=True)[0] == [0, 0]


def test_negative_slot_touches_nothing_and_slots_are_apart():
    a = np.array([1.0, 50.0, 1.0, 9.0, 2.0, 9.0]).reshape(-1, 1, 1)
    slot = [0, -1, 1, 0, 5, 1]                            # 5 >= slots: as a negative slot
    flag, m, age, margin = cmap_ref.recursion(a, T=4.0, w=0.5, warmup=1, hold=False, slot=slot, slots=2)
    assert flag[:, 0, 0].tolist() == [0, 0, 0, 1, 0, 1]
    assert m[:, 0, 0].tolist() == [5.0, 5.0] and age.tolist() == [2, 2]
    assert np.isinf(margin[1]).all() and np.isinf(margin[4]).all()
    # interleaved = the two slots run apart
    f0, m0, a0, _ = cmap_ref.recursion(a[[0, 3]], T=4.0, w=0.5, warmup=1, hold=False)
    assert f0[:, 0, 0].tolist() == [0, 1] and m0[0, 0, 0] == 5.0 and a0.tolist() == [2]
    # a state carried from call to call gives what one call gives
    fa, ma, aa, _ = cmap_ref.recursion(a[:3], T=4.0, w=0.5, warmup=1, hold=False, slot=slot[:3], slots=2)
    fb, mb, ab, _ = cmap_ref.recursion(a[3:], T=4.0, w=0.5, warmup=1, hold=False, slot=slot[3:], slots=2,
                                       state=(ma, aa))
    np.testing.assert_array_equal(np.concatenate([fa, fb]), flag)
    np.testing.assert_array_equal(mb, m)
    np.testing.assert_array_equal(ab, age)


def test_age_saturates():
    a = np.ones((2, 1, 1))
    state = (np.ones((1, 1, 1)), np.array([cmap_ref.AGE_MAX - 1]))
    _, _, age, _ = cmap_ref.recursion(a, T=4.0, w=0.5, warmup=1, hold=True, state=state)
    assert age.tolist() == [cmap_ref.AGE_MAX]


# ---------------------------------------------------------------- band_of and rows
def test_band_of_matches_the_mtd_zero_band():
    from rsp import cmap
    seen = set()
    for case in mtd_ref.CASES:
        key = (case.V, case.zdiv, case.zends)
        if key in seen:
            continue
        seen.add(key)
        zb = mtd_ref.zero_band(case.V, case.zdiv, case.zends)
        # zero_ends bands sit round row 0 of an unshifted RDM, zero_v_div bands round the centre
        # row of an fftshifted one: elsewhere the rows are not round zero velocity
        shift = 0 if case.zends else 1
        spec = types.SimpleNamespace(V=case.V, zero_v_div=case.zdiv, zero_ends=case.zends, fftshift=shift)
        if not zb.any():
            with pytest.raises(ValueError):
                cmap.band_of(spec)
            continue
        q_lo, q_hi = cmap.band_of(spec)
        got = np.zeros(case.V, bool)
        got[cmap.rows(q_lo, q_hi, case.V, shift)] = True
        np.testing.assert_array_equal(got, zb, err_msg=str(key))
        assert q_hi - q_lo + 1 == int(zb.sum())
        np.testing.assert_array_equal(cmap.rows(q_lo, q_hi, case.V, shift), cmap_ref.rows(q_lo, q_hi, case.V, shift))
        with pytest.raises(ValueError):
            spec.fftshift = 1 - shift
            cmap.band_of(spec)
    assert len(seen) > 20


def test_band_of_presets():
    from rsp import cmap, presets
    spec = presets.dmx(128, 4096)
    assert cmap.band_of(spec) == (-2, 0)                      # /150 at P = 128: off-centre, as the reference is
    assert cmap.band_of(spec, presets.default_cfar(spec)) == (-7, 5)      # main_cfar's /20 band: 13 rows
    assert cmap.rows(-7, 5, 128, 1).tolist() == list(range(57, 70))
    d = presets.dmx_native()
    m0 = d.radar["M0"]
    assert d.zero_ends == m0 + 1 and cmap.band_of(d) == (-m0, m0) == cmap.band_of(d, presets.default_cfar(d))
    assert cmap.rows(-2, 2, 2048, 0).tolist() == [2046, 2047, 0, 1, 2]


# ---------------------------------------------------------------- the designed scene, in fp64
@pytest.mark.parametrize("case", cmap_ref.CASES, ids=[c[0] for c in cmap_ref.CASES])
def test_scene_conditions(case):
    """What the GPU tests rely on, in the reference alone: every tone cell stands at a >= 2 T m,
    with hold, in each of its four frames; near-threshold cells are at most 0.1 % of the tested
    band cells; and without hold at w = 1/8 the map absorbs the tone inside the scene."""
    _, cells, a = cmap_ref.case_scene(case)
    w = case[8]
    assert len(cells) >= 1 and a.shape[0] == cmap_ref.F
    state = None
    for f in range(cmap_ref.F):
        if f >= cmap_ref.TONE_FROM:
            for k, col in cells:
                assert a[f, k, col] >= 2.0 * cmap_ref.T * state[0][0, k, col], (f, k, col)
        fl, m, age, _ = cmap_ref.recursion(a[f:f + 1], cmap_ref.T, w, cmap_ref.WARMUP, True, state=state)
        state = (m, age)
    for wq in (0.25, 0.125):
        flag, _, _, margin = cmap_ref.recursion(a, cmap_ref.T, wq, cmap_ref.WARMUP, True)
        tested = int(np.isfinite(margin).sum())
        assert tested == (cmap_ref.F - cmap_ref.WARMUP) * a.shape[1] * a.shape[2]
        assert int((margin < cmap_ref.NEAR_TOL).sum()) <= 1e-3 * tested
        for k, col in cells:
            assert flag[cmap_ref.TONE_FROM:, k, col].all()
    flag, _, _, _ = cmap_ref.recursion(a, cmap_ref.T, 0.125, cmap_ref.WARMUP, False)
    for k, col in cells:
        assert flag[cmap_ref.TONE_FROM, k, col] == 1 and flag[cmap_ref.F - 1, k, col] == 0


@pytest.mark.parametrize("P,V,K,beams", [(32, 32, 3, 1), (33, 64, 7, 1), (128, 128, 13, 1), (96, 128, 13, 2)])
def test_scene_conditions_small_shapes(P, V, K, beams):
    q_lo = -(K // 2)
    x, cells = cmap_ref.scene(P, V, 69, q_lo, q_lo + K - 1, mtd_ref.HAMMING, beams, seed=P)
    a = cmap_ref.scene_band(x, mtd_ref.HAMMING, P, V, q_lo, q_lo + K - 1, beams)
    for w in (0.25, 0.125):
        flag, _, _, margin = cmap_ref.recursion(a, 4.0, w, 4, True)
        assert int((margin < cmap_ref.NEAR_TOL).sum()) <= 1e-3 * int(np.isfinite(margin).sum())
        for k, col in cells:
            assert flag[cmap_ref.TONE_FROM:, k, col].all()


def test_tone_plan_straddles_group_boundaries():
    plan = cmap_ref.tone_plan(70, -32, 31, 16)
    assert [q for q, _ in plan] == [-32, -17, -16, -1, 0, 15, 16, 31]
    assert {c for _, c in plan} == set(cmap_ref.free_columns(70)) and len(cmap_ref.free_columns(70)) == 3
    assert [q for q, _ in cmap_ref.tone_plan(9, -2, 0, 4)] == [-2, 0]
    for R in (1, 2, 65, 66, 67, 69, 130, 200, 1100):
        c = cmap_ref.clutter_phase(R)
        assert all(r % 3 != c and 0 <= r < R for r in cmap_ref.free_columns(R))


# ---------------------------------------------------------------- the C boundary
def _lib():
    from rsp import _capi
    return _capi, _capi.load_library()


def test_header_declares_and_library_exports():
    _capi, lib = _lib()
    text = open(os.path.join(ROOT, "include", "rsp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("rsp_cmap_dev", "rsp_cmap_plan"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text)
        assert hasattr(lib, name) and name in _capi.EXPORTS
    assert re.search(r"#define\s+RSP_CMAP_MAX_BINS\s+64\b", text) and _capi.RSP_CMAP_MAX_BINS == 64


@pytest.mark.parametrize("struct", ["rsp_cmap_params", "rsp_cmap_plan_t"])
def test_struct_layout_matches_header(struct):
    _capi, _ = _lib()
    cls = getattr(_capi, struct)
    fields = [n for n, _ in cls._fields_]
    src = ('#include "rsp.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%%zu", sizeof(%s));\n' % struct
           + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields)
           + 'printf(" %d\\n", RSP_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    want = [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields] + [5]
    assert got == want


def _params(_capi, P=128, V=0, beams=1, window=0, beta=8.0, q=(-2, 0), warmup=4, hold=1, T=4.0, w=0.25, ld=0, cs=0):
    p = _capi.rsp_cmap_params()
    p.P, p.V, p.beams, p.window, p.window_beta = P, V, beams, window, beta
    p.q_lo, p.q_hi, p.warmup, p.hold, p.T, p.w, p.ld, p.cpi_stride = q[0], q[1], warmup, hold, T, w, ld, cs
    return p


def test_plan_reports_the_sweep_instances():
    """Every instance the plan can report is one the sweep table names (no GPU needed: the plan
    is a function of its arguments, and takes a NULL context)."""
    _capi, lib = _lib()
    seen = set()
    for cid, P, V, beams, q, R, ld, window, w, inst in cmap_ref.CASES:
        out = _capi.rsp_cmap_plan_t()
        p = _params(_capi, P=P, V=V, beams=beams, window=window, q=q, w=w, ld=ld)
        assert lib.rsp_cmap_plan(None, R, cmap_ref.F, C.byref(p), C.byref(out)) == 0, cid
        K = q[1] - q[0] + 1
        assert (out.bins_per_pass, out.vec, out.split) == inst, cid
        assert out.K == K and out.passes == -(-K // out.bins_per_pass) and out.kpad == out.passes * out.bins_per_pass
        assert out.threads == 64 * out.split and out.table_bytes == P * out.kpad * 8
        assert out.pool_bytes == cmap_ref.F * K * R * 4
        seen.add(inst)
    assert seen == {(kb, vec, split) for kb in (4, 16) for vec in (1, 2) for split in (1, 4)}
    # the split follows R and P alone: the batch never changes it
    for batch in (0, 1, 7, 4096):
        out = _capi.rsp_cmap_plan_t()
        p = _params(_capi, P=1536, V=2048, beams=2, q=(-6, 6), ld=574)
        assert lib.rsp_cmap_plan(None, 566, batch, C.byref(p), C.byref(out)) == 0
        assert (out.bins_per_pass, out.passes, out.vec, out.split) == (16, 1, 2, 4)
    # an overlapping-window stride that is odd takes the 8-byte path
    out = _capi.rsp_cmap_plan_t()
    p = _params(_capi, P=128, q=(-2, 0), ld=64, cs=33 * 64 + 1)
    assert lib.rsp_cmap_plan(None, 64, 2, C.byref(p), C.byref(out)) == 0 and out.vec == 1


def test_null_and_malformed_arguments():
    """Everything is refused before the context is looked at: no GPU needed (ctx == NULL; the
    addresses are never touched)."""
    _capi, lib = _lib()
    pc, slot, dmap, age, band, flag = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000

    def call(p, pc=pc, slot=slot, dmap=dmap, age=age, band=band, flag=flag, R=20, B=3, slots=2):
        return lib.rsp_cmap_dev(None, pc, R, B, C.byref(p) if p is not None else None, slot, slots, dmap, age, band,
                                flag, None)

    def msg():
        return lib.rsp_last_error(None).decode()

    ARG = _capi.RSP_ERR_ARG
    P = lambda **kw: _params(_capi, **kw)   # noqa: E731
    # a well-formed call gets as far as the null context; d_slot and d_band may be NULL
    assert call(P()) == ARG and "null ctx" in msg()
    assert call(P(), slot=None, band=None) == ARG and "null ctx" in msg()
    assert call(P(P=2, q=(0, 0))) == ARG and "null ctx" in msg()                      # any P >= 2
    assert call(P(P=1536, V=2048, beams=2, window=1, q=(-32, 31), ld=24, cs=7)) == ARG and "null ctx" in msg()
    assert call(P(P=33, V=64, q=(5, 9), warmup=0, hold=0, w=1.0)) == ARG and "null ctx" in msg()   # 0 outside the band
    for kw in (dict(pc=None), dict(dmap=None), dict(age=None), dict(flag=None)):
        assert call(P(), **kw) == ARG and "null argument" in msg(), kw
    assert call(None) == ARG and "null argument" in msg()
    # K out of range
    assert call(P(q=(1, 0))) == ARG and "bins" in msg()
    assert call(P(P=512, q=(-32, 32))) == ARG and "outside 1..64" in msg()
    assert call(P(P=512, q=(-32, 31))) == ARG and "null ctx" in msg()
    # |q| < V/2
    assert call(P(P=16, q=(-8, 0))) == ARG and "V/2" in msg()
    assert call(P(P=16, q=(-7, 7))) == ARG and "null ctx" in msg()
    assert call(P(P=17, q=(0, 9))) == ARG and "V/2" in msg()
    assert call(P(P=17, q=(-8, 8))) == ARG and "null ctx" in msg()
    assert call(P(P=2, q=(0, 1))) == ARG and "V/2" in msg()
    assert call(P(P=10, V=64, q=(-20, 20))) == ARG and "null ctx" in msg()             # V, not P, bounds q
    # w outside (0, 1], T, warmup, hold
    for w in (0.0, -0.25, 1.0 + 1e-9, float("nan")):
        assert call(P(w=w)) == ARG and "w =" in msg(), w
    for T in (0.0, -1.0, float("inf"), float("nan")):
        assert call(P(T=T)) == ARG and "threshold" in msg(), T
    assert call(P(warmup=-1)) == ARG and "warmup" in msg()
    assert call(P(hold=2)) == ARG and "hold" in msg()
    # shape
    assert call(P(P=1, q=(0, 0))) == ARG and "bad P" in msg()
    assert call(P(P=128, V=64)) == ARG and "bad P" in msg()
    assert call(P(beams=3)) == ARG and "beams" in msg()
    assert call(P(window=3)) == ARG and "window" in msg()
    assert call(P(), R=0) == ARG and "bad shape" in msg()
    assert call(P(), B=-1) == ARG and "bad shape" in msg()
    assert call(P(), slots=0) == ARG and "slots" in msg()
    assert call(P(ld=19)) == ARG and "row pitch" in msg()
    assert call(P(ld=20)) == ARG and "null ctx" in msg()
    assert call(P(cs=-5)) == ARG and "CPI stride" in msg()
    # the plan refuses the same
    out = _capi.rsp_cmap_plan_t()
    p = P(q=(1, 0))
    assert lib.rsp_cmap_plan(None, 20, 3, C.byref(p), C.byref(out)) == ARG and "bins" in msg()
    assert lib.rsp_cmap_plan(None, 20, 3, None, C.byref(out)) == ARG
    p = P()
    assert lib.rsp_cmap_plan(None, 20, 3, C.byref(p), None) == ARG
