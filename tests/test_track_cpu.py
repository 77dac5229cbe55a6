"""Tracking, CPU side: the restatement tests/track_ref.py against hand-computed CPIs, its two forms
of the association against each other, the designed scene's conditions, and the C ABI's
declaration, struct layout and refusals (rsp_track_dev checks everything it can before it looks at
the context).
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _walk(p, cpis, slots=1):
    """Apply CPIs (lists of (r, v, ele)) one at a time to a fresh slot; returns the state and the
    list of (assign, tcount) per CPI."""
    state = tr.new_state(slots, p.max_tracks)
    outs = []
    for plots in cpis:
        est = np.asarray(plots, np.float64).reshape(-1, 3)
        outs.append(tr.step(state[0][0], state[1][0], state[2][0], est, len(est), p))
    return state, outs


def _entry(state, t):
    return state[0][0, t].tolist(), state[1][0, t].tolist()


def _still(r, n, ele=0.0):
    return [[(r, 0.0, ele)]] * n


# ---------------------------------------------------------------- the steps by hand
def test_one_track_hit_miss_hit_every_field():
    p = tr.Params(max_tracks=2, confirm=(3, 5), drop=(3, 4), dt=0.5, gate=(10.0, 2.0), alpha=(0.5, 0.25, 0.5))
    state = tr.new_state(1, 2)
    sf, si, meta = state[0][0], state[1][0], state[2][0]

    a, tc = tr.step(sf, si, meta, [(100.0, 4.0, 1.0)], 1, p)
    assert sf[0].tolist() == [100.0, 4.0, 1.0, 0.0] and si[0].tolist() == [1, 1, 1, 0, 1, 1, 0, 0]
    assert a.tolist() == [1] and tc.tolist() == [1, 0, 1, 0, 0, 1, 0, 0] and meta.tolist() == [1, 1]
    assert not si[1].any() and not sf[1].any()

    # rp = 100 + (1*4)*0.5 = 102: dr = 2, dv = 2 (on the gate, which is inside)
    a, tc = tr.step(sf, si, meta, [(104.0, 6.0, 3.0)], 1, p)
    assert sf[0].tolist() == [103.0, 4.5, 2.0, 0.0] and si[0].tolist() == [1, 1, 3, 0, 2, 2, 0, 0]
    assert a.tolist() == [1] and tc.tolist() == [1, 0, 0, 0, 0, 1, 1, 0] and meta.tolist() == [1, 2]

    # no plot: the track coasts to rp = 103 + 4.5*0.5
    a, tc = tr.step(sf, si, meta, np.zeros((0, 3)), 0, p)
    assert sf[0].tolist() == [105.25, 4.5, 2.0, 0.0] and si[0].tolist() == [1, 1, 6, 1, 2, 3, -1, 0]
    assert a.tolist() == [] and tc.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and meta.tolist() == [1, 3]

    # rp = 107.5, dr = -0.25; a NaN ele leaves the track's; hist 0b1101 has three hits in five: confirmed
    a, tc = tr.step(sf, si, meta, [(107.25, 4.5, NAN)], 1, p)
    assert sf[0].tolist() == [107.375, 4.5, 2.0, 0.0] and si[0].tolist() == [1, 2, 13, 0, 3, 4, 0, 0]
    assert a.tolist() == [1] and tc.tolist() == [1, 1, 0, 0, 0, 1, 1, 0] and meta.tolist() == [1, 4]


def test_rate_sign_and_dt_per_cpi():
    p = tr.Params(max_tracks=1, dt=0.5, rate_sign=-1.0, gate=(10.0, 2.0), confirm=(5, 5), drop=(5, 5))
    state = tr.new_state(1, 1)
    sf, si, meta = state[0][0], state[1][0], state[2][0]
    tr.step(sf, si, meta, [(100.0, 4.0, 0.0)], 1, p)
    tr.step(sf, si, meta, np.zeros((0, 3)), 0, p)
    assert sf[0, 0] == 98.0
    tr.step(sf, si, meta, np.zeros((0, 3)), 0, p, h=0.25)
    assert sf[0, 0] == 97.0


def test_two_of_three_confirms_before_the_age_rule():
    p = tr.Params(max_tracks=2, confirm=(2, 3), drop=(2, 4), gate=(10.0, 2.0))
    state, outs = _walk(p, [[(100.0, 0.0, 0.0)], [], [(100.0, 0.0, 0.0)]])
    # start (hist 1), miss (hist 2), hit (hist 5): two of the last three at age 3 = N, confirmed first
    assert _entry(state, 0)[1] == [1, 2, 5, 0, 2, 3, 0, 0]
    assert [o[1][tr.NCONF] for o in outs] == [0, 0, 1]


def test_tentative_deleted_at_age_n():
    p = tr.Params(max_tracks=2, confirm=(3, 4), drop=(5, 5), gate=(10.0, 2.0))
    state, outs = _walk(p, [[(100.0, 0.0, 0.0)], [(100.0, 0.0, 0.0)], [], []])
    # hist 0b1100 at age 4 = N: two hits of four, two misses < 5, deleted all the same
    assert [o[1][tr.DROPPED] for o in outs] == [0, 0, 0, 1] and [o[1][tr.LIVE] for o in outs] == [1, 1, 1, 0]
    assert not state[0].any() and not state[1].any() and state[2][0].tolist() == [1, 4]


def test_both_drop_counts():
    p = tr.Params(max_tracks=2, confirm=(3, 5), drop=(2, 3), gate=(10.0, 2.0))
    _, outs = _walk(p, [[(100.0, 0.0, 0.0)], [], []])
    assert [o[1][tr.DROPPED] for o in outs] == [0, 0, 1]           # tentative: two misses, at age 3 < 5
    p = tr.Params(max_tracks=2, confirm=(2, 5), drop=(2, 3), gate=(10.0, 2.0))
    state, outs = _walk(p, _still(100.0, 2) + [[], [], []])
    assert [o[1][tr.NCONF] for o in outs] == [0, 1, 1, 1, 0]          # confirmed: two misses keep it,
    assert [o[1][tr.DROPPED] for o in outs] == [0, 0, 0, 0, 1]        # the third deletes it
    assert not state[1].any()


def test_cost_tie_between_two_tracks_goes_to_the_lower_entry():
    p = tr.Params(max_tracks=4, gate=(30.0, 2.0))
    state, outs = _walk(p, [[(100.0, 0.0, 0.0), (120.0, 0.0, 0.0)], [(110.0, 0.0, 0.0)]])
    assert outs[1][0].tolist() == [1] and outs[1][1][tr.MATCHED] == 1 and outs[1][1][tr.STARTED] == 0
    assert _entry(state, 0) == ([105.0, 0.0, 0.0, 0.0], [1, 1, 3, 0, 2, 2, 0, 0])
    assert _entry(state, 1) == ([120.0, 0.0, 0.0, 0.0], [2, 1, 2, 1, 1, 2, -1, 0])


def test_cost_tie_between_two_plots_goes_to_the_lower_plot():
    p = tr.Params(max_tracks=4, gate=(30.0, 2.0))
    state, outs = _walk(p, [[(100.0, 0.0, 0.0)], [(105.0, 0.0, 1.0), (105.0, 0.0, 2.0)]])
    assert outs[1][0].tolist() == [1, 2]
    assert _entry(state, 0) == ([102.5, 0.0, 0.5, 0.0], [1, 1, 3, 0, 2, 2, 0, 0])
    assert _entry(state, 1) == ([105.0, 0.0, 2.0, 0.0], [2, 1, 1, 0, 1, 1, 1, 0])


def test_confirmed_track_beats_a_closer_tentative_one():
    p = tr.Params(max_tracks=4, confirm=(2, 5), gate=(30.0, 2.0))
    state, outs = _walk(p, [[(100.0, 0.0, 0.0)], [(100.0, 0.0, 0.0)], [(100.0, 0.0, 0.0), (112.0, 0.0, 0.0)],
                            [(110.0, 0.0, 0.0)]])
    assert outs[2][0].tolist() == [1, 2] and state[1][0, 0, tr.STATUS] == 2 and state[1][0, 1, tr.STATUS] == 1
    assert outs[3][0].tolist() == [1]                       # dr = 10 for the confirmed, -2 for the tentative
    assert state[0][0, 0, 0] == 105.0 and state[1][0, 1].tolist() == [2, 1, 2, 1, 1, 2, -1, 0]


def test_nan_plot_is_invalid():
    p = tr.Params(max_tracks=4, gate=(30.0, 2.0))
    _, outs = _walk(p, [[(NAN, 1.0, 0.0), (100.0, 0.0, 0.0), (5.0, NAN, 0.0)]])
    assert outs[0][0].tolist() == [-1, 1, -1] and outs[0][1].tolist() == [1, 0, 1, 0, 0, 1, 0, 0]


def test_nan_ele():
    p = tr.Params(max_tracks=2, gate=(30.0, 2.0), confirm=(5, 5), drop=(3, 3))
    state, _ = _walk(p, [[(100.0, 0.0, NAN)]])
    assert np.isnan(state[0][0, 0, 2])
    state, _ = _walk(p, [[(100.0, 0.0, NAN)], [(100.0, 0.0, 3.0)]])
    assert state[0][0, 0, 2] == 3.0                          # the plot's, not a blend with NaN
    state, _ = _walk(p, [[(100.0, 0.0, NAN)], [(100.0, 0.0, 3.0)], [(100.0, 0.0, NAN)], [(100.0, 0.0, 5.0)]])
    assert state[0][0, 0, 2] == 4.0 and state[1][0, 0, tr.HITS] == 4


def test_table_overflow():
    p = tr.Params(max_tracks=2, gate=(30.0, 2.0))
    state, outs = _walk(p, [[(100.0, 0.0, 0.0), (500.0, 0.0, 0.0), (900.0, 0.0, 0.0)]])
    assert outs[0][0].tolist() == [1, 2, 0]
    assert outs[0][1].tolist() == [2, 0, 2, 0, 1, 3, 0, 0] and state[2][0].tolist() == [2, 1]


def test_freed_entries_are_reused_in_index_order():
    p = tr.Params(max_tracks=2, confirm=(3, 5), drop=(1, 1), gate=(30.0, 2.0))
    state, outs = _walk(p, [[(100.0, 0.0, 0.0), (500.0, 0.0, 0.0)], [(500.0, 0.0, 0.0), (900.0, 0.0, 0.0)]])
    # entry 0 misses and is deleted, and the new plot takes it in the same CPI
    assert outs[1][0].tolist() == [2, 3] and outs[1][1].tolist() == [2, 0, 1, 1, 0, 2, 1, 0]
    assert state[1][0, 0].tolist() == [3, 1, 1, 0, 1, 1, 1, 0]


def test_m_equals_one():
    p = tr.Params(max_tracks=2, confirm=(1, 1), drop=(1, 1), gate=(30.0, 2.0))
    state, outs = _walk(p, [[(100.0, 0.0, 0.0)], []])
    assert outs[0][1].tolist() == [1, 1, 1, 0, 0, 1, 0, 0]   # confirmed as it starts
    assert outs[1][1].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and not state[1].any()


def test_n_equals_32():
    p = tr.Params(max_tracks=2, confirm=(32, 32), drop=(40, 40), gate=(30.0, 2.0))
    state, outs = _walk(p, _still(100.0, 33))
    assert [o[1][tr.NCONF] for o in outs] == [0] * 31 + [1, 1]
    assert state[1][0, 0].tolist() == [1, 2, -1, 0, 33, 33, 0, 0]      # hist 0xffffffff
    _, outs = _walk(p, _still(100.0, 10) + [[]] + _still(100.0, 21))
    assert [o[1][tr.DROPPED] for o in outs] == [0] * 31 + [1]           # 31 of 32 at age 32


# ---------------------------------------------------------------- two forms of the association
def test_mutual_best_rounds_equal_the_sequential_greedy():
    deepest = {}
    for case in tr.CASES:
        cid, p = case[0], case[1]
        est, count, dt = tr.case_inputs(case)
        rounds = [0]

        def by_rounds(cands, T, n):
            m, k = tr.associate_rounds(cands, T, n)
            rounds[0] = max(rounds[0], k)
            return m

        sa, sb = tr.new_state(1, p.max_tracks), tr.new_state(1, p.max_tracks)
        oa = tr.run(sa, est, count, p, dt=dt)
        ob = tr.run(sb, est, count, p, dt=dt, associate=by_rounds)
        for x, y in zip(oa + sa, ob + sb):
            assert x.tobytes() == y.tobytes(), cid
        deepest[cid] = rounds[0]
    # the tie-heavy scenes are there to make the matching take several rounds
    assert deepest["t64_quant"] >= 3 and max(deepest.values()) <= 8, deepest


def test_cases_cover_the_shapes():
    ids = [c[0] for c in tr.CASES]
    assert len(set(ids)) == len(ids)
    assert {c[1].max_tracks for c in tr.CASES} == {1, 5, 64, 65, 256, 1024}
    plots = set()
    for case in tr.CASES:
        est, count, _ = tr.case_inputs(case)
        assert 12 <= est.shape[0] <= 40
        plots |= {int(x) for x in count[:, 0]}
        if case[0] == "t1024_p1100":
            assert est.shape[1] == 1024 and (count[:, 0] == 1100).all()
    assert {0, 1, 63, 64, 65, 300, 1100} <= plots
    assert {c[1].rate_sign for c in tr.CASES} == {1.0, -1.0} and {c[3] for c in tr.CASES} == {False, True}
    assert any(c[1].M == 1 for c in tr.CASES) and any(c[1].N == 32 for c in tr.CASES)


# ---------------------------------------------------------------- the designed scene
@pytest.mark.parametrize("seed", [101, 202, 303])
def test_property_scene(seed):
    """4 constant-velocity targets in 20 false alarms per CPI: from the 11th CPI on each target has
    a confirmed track within 15 m and 1 m/s in at least 95 % of the CPIs, confirmed tracks near no
    target average at most 0.5 per CPI, and nothing overflows."""
    p = tr.Params(max_tracks=64, confirm=(3, 5), drop=(2, 4), dt=0.08, gate=(30.0, 2.0), alpha=(0.5, 0.5, 0.5))
    est, count, truth = tr.scene(seed, cpis=60, targets=4, false_alarms=20, dt=0.08, pd=0.9, sigma=(3.0, 0.2),
                                 span=(3000.0, 60.0))
    state = tr.new_state(1, 64)
    _, snap_f, snap_i, tcount = tr.run(state, est, count, p)
    assert (tcount[:, tr.NOT_STARTED] == 0).all() and tcount[:, tr.LIVE].max() < 64
    held = np.zeros((60, 4), bool)
    stray = 0
    for b in range(60):
        conf = np.flatnonzero(snap_i[b, :, tr.STATUS] == tr.CONFIRMED)
        near = (np.abs(snap_f[b, conf, 0][:, None] - truth[b, :, 0][None]) <= 15.0) & \
               (np.abs(snap_f[b, conf, 1][:, None] - truth[b, :, 1][None]) <= 1.0)
        held[b] = near.any(0)
        stray += int((~near.any(1)).sum())
    print("seed %d: held %s of 50, stray confirmed %.3f per CPI, most live %d"
          % (seed, held[10:].sum(0).tolist(), stray / 60.0, int(tcount[:, tr.LIVE].max())))
    assert (held[10:].mean(0) >= 0.95).all()
    assert stray / 60.0 <= 0.5


# ---------------------------------------------------------------- the C boundary
def _lib():
    from rsp import _capi
    return _capi, _capi.load_library()


def test_header_declares_and_library_exports():
    _capi, lib = _lib()
    text = open(os.path.join(ROOT, "include", "rsp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+rsp_track_dev\s*\(", text)
    assert hasattr(lib, "rsp_track_dev") and "rsp_track_dev" in _capi.EXPORTS
    assert re.search(r"#define\s+RSP_TRACK_MAX_TRACKS\s+1024\b", text) and _capi.RSP_TRACK_MAX_TRACKS == 1024


def test_struct_layout_matches_header():
    _capi, _ = _lib()
    struct, cls = "rsp_track_params", _capi.rsp_track_params
    fields = [n for n, _ in cls._fields_]
    src = ('#include "rsp.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%%zu", sizeof(%s));\n' % struct
           + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields)
           + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert fields == ["max_tracks", "confirm_m", "confirm_n", "drop_tentative", "drop_confirmed", "reserved", "dt",
                      "rate_sign", "gate_r", "gate_v", "alpha_r", "alpha_v", "alpha_e"]


def test_null_and_malformed_arguments():
    """Everything is refused before the context is looked at: no GPU needed (ctx == NULL; the
    addresses are never touched)."""
    _capi, lib = _lib()
    base = dict(est=1 << 40, count=2 << 40, slot=3 << 40, dt=4 << 40, sf=5 << 40, si=6 << 40, meta=7 << 40,
                assign=8 << 40, snf=9 << 40, sni=10 << 40, tc=11 << 40)

    def call(p, H=16, B=3, slots=2, **kw):
        a = dict(base, **kw)
        return lib.rsp_track_dev(None, a["est"], a["count"], H, B, C.byref(p) if p is not None else None, a["slot"],
                                 a["dt"], slots, a["sf"], a["si"], a["meta"], a["assign"], a["snf"], a["sni"], a["tc"],
                                 None)

    def msg():
        return lib.rsp_last_error(None).decode()

    ARG = _capi.RSP_ERR_ARG
    P = lambda **kw: tr.track_params(_capi, **kw)   # noqa: E731
    # a well-formed call gets as far as the null context; d_slot, d_dt and the snapshots may be NULL
    assert call(P()) == ARG and "null ctx" in msg()
    assert call(P(), slot=None, dt=None, snf=None, sni=None) == ARG and "null ctx" in msg()
    assert call(P(max_tracks=1, confirm=(1, 1), drop=(1, 1), rate_sign=-1.0, alpha=(1.0, 1.0, 1.0))) == ARG \
        and "null ctx" in msg()
    assert call(P(max_tracks=1024, confirm=(32, 32)), H=1024) == ARG and "null ctx" in msg()
    assert call(P(), H=0, est=None, assign=None) == ARG and "null ctx" in msg()
    for kw in (dict(est=None), dict(count=None), dict(sf=None), dict(si=None), dict(meta=None), dict(assign=None),
               dict(tc=None)):
        assert call(P(), **kw) == ARG and "null argument" in msg(), kw
    assert call(None) == ARG and "null argument" in msg()
    assert call(P(), snf=None) == ARG and "go together" in msg()
    assert call(P(), sni=None) == ARG and "go together" in msg()
    for kw, word in tr.BAD_PARAMS:
        assert call(P(**kw)) == ARG and word in msg(), kw
    assert call(P(), H=-1) == ARG and "bad shape" in msg()
    assert call(P(), B=-1) == ARG and "bad shape" in msg()
    assert call(P(), slots=0) == ARG and "slots" in msg()
    assert call(P(), slots=65536) == ARG and "slots" in msg()
    assert call(P(), est=(1 << 40) + 4) == ARG and "misaligned" in msg()
    assert call(P(), tc=(11 << 40) + 2) == ARG and "misaligned" in msg()
    # no buffer may overlap another: the snapshot inside the state, the assign row inside est
    assert call(P(), snf=(5 << 40) + 32) == ARG and "overlap" in msg()
    assert call(P(), assign=(1 << 40) + 8) == ARG and "overlap" in msg()
    assert call(P(), si=(5 << 40) + 2 * 64 * 32 - 4) == ARG and "overlap" in msg()
    assert call(P(), si=(5 << 40) + 2 * 64 * 32) == ARG and "null ctx" in msg()
    # the table and a CPI's plots must fit the LDS
    assert call(P(max_tracks=256), H=4656) == ARG and "null ctx" in msg()
    assert call(P(max_tracks=256), H=4657) == _capi.RSP_ERR_UNSUPPORTED and "LDS" in msg()
    assert call(P(max_tracks=1024), H=3313) == _capi.RSP_ERR_UNSUPPORTED and "LDS" in msg()
