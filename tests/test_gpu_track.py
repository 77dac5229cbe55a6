"""Tracking on the GPU (rsp_track_dev, csrc/rsp_track.hip) against the fp64 restatement
tests/track_ref.py.  The kernel does the same IEEE operations in the same order, so nothing has a
tolerance: integers are compared exactly and doubles bit for bit (through their bytes), NaN ele
included, with no allowance for ties.
"""
import ctypes as C
import os

import numpy as np
import pytest

import track_ref as tr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_REF = {}


def _ref(case):
    """(est, count, dt, outputs, final state) of a CASES row, computed once."""
    if case[0] not in _REF:
        est, count, dt = tr.case_inputs(case)
        state = tr.new_state(1, case[1].max_tracks)
        outs = tr.run(state, est, count, case[1], dt=dt)
        for a in outs + state:
            a.setflags(write=False)
        _REF[case[0]] = (est, count, dt, outs, state)
    return _REF[case[0]]


def _tracker(p, slots=1):
    from rsp.track import Tracker
    return Tracker(0, slots=slots, **p.kwargs())


def _update(trk, est, count, **kw):
    import torch
    out = trk.update_dev(torch.from_numpy(np.ascontiguousarray(est)).cuda(),
                         torch.from_numpy(np.ascontiguousarray(count)).cuda(), **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _state(trk):
    return tuple(t.cpu().numpy() for t in trk.state())


def _same(got, want, what):
    names = ("assign", "snap_f", "snap_i", "tcount") if len(got) == 4 else ("state_f", "state_i", "meta")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.int64 if g.dtype == np.float64 else np.int32) !=
                              w.view(np.int64 if w.dtype == np.float64 else np.int32))
            raise AssertionError("%s: %s differs at %d places, first %s: got %r, want %r"
                                 % (what, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


@pytest.mark.parametrize("case", tr.CASES, ids=[c[0] for c in tr.CASES])
def test_cases_match_the_restatement(case):
    est, count, dt, want, want_state = _ref(case)
    trk = _tracker(case[1])
    try:
        got = _update(trk, est, count, dt=dt)
        _same(got, want, case[0])
        _same(_state(trk), want_state, case[0])
    finally:
        trk.close()


def _case(cid):
    return next(c for c in tr.CASES if c[0] == cid)


@pytest.mark.parametrize("cid", ["t64_p64", "t64_quant", "t5_p63_overflow"])
def test_one_batch_equals_batches_of_one_and_a_second_run(cid):
    case = _case(cid)
    est, count, dt, want, want_state = _ref(case)
    trk = _tracker(case[1])
    try:
        one = _update(trk, est, count, dt=dt)
        s_one = _state(trk)
        trk.reset()
        again = _update(trk, est, count, dt=dt)
        _same(again, one, "second run")
        _same(_state(trk), s_one, "second run")
        trk.reset()
        parts = [_update(trk, est[b:b + 1], count[b:b + 1], dt=None if dt is None else dt[b:b + 1])
                 for b in range(est.shape[0])]
        _same(tuple(np.concatenate([q[i] for q in parts]) for i in range(4)), one, "batches of one")
        _same(_state(trk), s_one, "batches of one")
        # a split in the middle, and no snapshot: the other outputs and the state do not change
        trk.reset()
        h = est.shape[0] // 2
        a = _update(trk, est[:h], count[:h], dt=None if dt is None else dt[:h], snapshot=False)
        b = _update(trk, est[h:], count[h:], dt=None if dt is None else dt[h:], snapshot=False)
        assert a[1] is None and a[2] is None
        assert np.concatenate([a[0], b[0]]).tobytes() == one[0].tobytes()
        assert np.concatenate([a[3], b[3]]).tobytes() == one[3].tobytes()
        _same(_state(trk), s_one, "snapshot=False")
        _same(one, want, cid)
    finally:
        trk.close()


def test_interleaved_slots_and_slots_out_of_range():
    """Two scenes interleaved CPI by CPI on two slots of three, with CPIs of slot -1 and slot 3 in
    between: each slot's outputs and state are those of its scene alone, the out-of-range CPIs
    write zero snapshots and their valid counts, and the third slot stays zero."""
    ca, cb = _case("t64_p64"), _case("t64_quant")
    pa = ca[1]
    ea, na, _, _, _ = _ref(ca)
    eb, nb = tr.quantised_scene(21, cpis=ea.shape[0], plots=40, max_hits=ea.shape[1])
    B, H = ea.shape[0], ea.shape[1]
    est = np.full((3 * B, H, 3), np.nan)
    count = np.zeros((3 * B, 2), np.int32)
    slot = np.zeros(3 * B, np.int32)
    est[0::3], count[0::3], slot[0::3] = ea, na, 1
    est[1::3], count[1::3], slot[1::3] = eb, nb, 0
    est[2::3], count[2::3] = ea, na
    slot[2::3] = np.where(np.arange(B) % 2 == 0, -1, 3)
    est[2, 0, 0] = np.nan                       # an invalid plot in an out-of-range CPI
    want_a = tr.run(tr.new_state(1, pa.max_tracks), ea, na, pa)
    sb = tr.new_state(1, pa.max_tracks)
    want_b = tr.run(sb, eb, nb, pa)
    trk = _tracker(pa, slots=3)
    try:
        got = _update(trk, est, count, slot=slot)
        _same(tuple(g[0::3] for g in got), want_a, "slot 1")
        _same(tuple(g[1::3] for g in got), want_b, "slot 0")
        off = tuple(g[2::3] for g in got)
        assert not off[1].any() and not off[2].any()
        valid = ~(np.isnan(est[2::3, :, 0]) | np.isnan(est[2::3, :, 1]))
        n = np.minimum(count[2::3, 0], H)
        live = np.arange(H)[None, :] < n[:, None]
        np.testing.assert_array_equal(off[0], np.where(live & ~valid, -1, 0))
        want_tc = np.zeros((B, 8), np.int32)
        want_tc[:, tr.N_VALID] = (live & valid).sum(1)
        np.testing.assert_array_equal(off[3], want_tc)
        assert off[0][0, 0] == -1
        sf, si, meta = _state(trk)
        _same((sf[0:1], si[0:1], meta[0:1]), sb, "slot 0")
        assert not sf[2].any() and not si[2].any() and not meta[2].any()
        assert meta[1].tolist() == [int(want_a[3][:, tr.STARTED].sum()), B]
        # the whole interleaved batch against the restatement with slots, and reset of one slot
        s3 = tr.new_state(3, pa.max_tracks)
        _same(got, tr.run(s3, est, count, pa, slot=slot), "three slots")
        _same((sf, si, meta), s3, "three slots")
        trk.reset(1)
        sf, si, meta = _state(trk)
        assert not sf[1].any() and not si[1].any() and not meta[1].any() and meta[0, 1] == B
        conf = trk.confirmed(0)
        k = np.flatnonzero(s3[1][0, :, tr.STATUS] == tr.CONFIRMED)
        np.testing.assert_array_equal(conf["id"], s3[1][0, k, tr.ID])
        assert conf["r"].tobytes() == s3[0][0, k, 0].tobytes() and len(k) > 0
    finally:
        trk.close()


def test_refusals_with_a_context():
    """RSP_ERR_ARG for each bad parameter, with a real context and real buffers; nothing is written."""
    import torch
    from rsp import _capi
    case = _case("t5_p0")
    trk = _tracker(case[1])
    try:
        B, H, T = 2, 4, case[1].max_tracks
        est = torch.zeros((B, H, 3), dtype=torch.float64, device="cuda")
        count = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
        assign = torch.full((B, H), 77, dtype=torch.int32, device="cuda")
        tcount = torch.full((B, 8), 77, dtype=torch.int32, device="cuda")

        def call(p, **kw):
            a = dict(est=est.data_ptr(), count=count.data_ptr(), H=H, B=B, slots=1, sf=trk.state_f.data_ptr(),
                     si=trk.state_i.data_ptr(), meta=trk.meta.data_ptr(), assign=assign.data_ptr(), tc=tcount.data_ptr())
            a.update(kw)
            return trk.lib.rsp_track_dev(trk.ctx, a["est"], a["count"], a["H"], a["B"], C.byref(p), None, None,
                                         a["slots"], a["sf"], a["si"], a["meta"], a["assign"], None, None, a["tc"], None)

        def msg():
            return trk.lib.rsp_last_error(trk.ctx).decode()

        for kw, word in tr.BAD_PARAMS:
            p = tr.track_params(_capi, **dict(dict(max_tracks=T), **kw))
            assert call(p) == _capi.RSP_ERR_ARG and word in msg(), kw
        good = tr.track_params(_capi, max_tracks=T)
        assert call(good, slots=0) == _capi.RSP_ERR_ARG and "slots" in msg()
        assert call(good, H=-1) == _capi.RSP_ERR_ARG and "bad shape" in msg()
        assert call(good, meta=None) == _capi.RSP_ERR_ARG and "null argument" in msg()
        assert call(good, assign=est.data_ptr()) == _capi.RSP_ERR_ARG and "overlap" in msg()
        assert call(good, H=6000) == _capi.RSP_ERR_UNSUPPORTED and "LDS" in msg()
        torch.cuda.synchronize()
        assert (assign == 77).all() and (tcount == 77).all() and not trk.meta.any()
        assert call(good) == _capi.RSP_OK
        torch.cuda.synchronize()
        assert not assign.any() and trk.meta.cpu().numpy().tolist() == [[0, 2]]
    finally:
        trk.close()


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


TRACK = dict(gate=(60.0, 3.0), alpha=(0.5, 0.5, 0.25), confirm=(2, 3), drop=(2, 3), max_tracks=64)


@pytest.mark.parametrize("condense", [None, dict(gap=(1, 1))], ids=["hits", "plots"])
def test_process_dev_tracks(dmx, condense):
    """process_dev(track=...): each key's tracks equal the restatement fed that call's (est, count),
    every other output equals the track=None call's bytes, and a second call continues the first
    one's state as one call over both batches does."""
    import torch
    proc, echo = dmx
    pairs = [(p, k) for p in ("short", "long") for k in ("flag", "flagV")]
    base = proc.process_dev(echo, 4, condense=condense, max_hits=512)
    proc.reset_tracks()
    out1 = proc.process_dev(echo, 4, condense=condense, max_hits=512, track=TRACK)
    out2 = proc.process_dev(echo.flip(0), 4, condense=condense, max_hits=512, track=TRACK)
    torch.cuda.synchronize()
    two_calls = _state(proc._tracker)
    assert set(out1) == set(base) | {(p, k, "tracks") for p, k in pairs}
    for k in base:
        if not isinstance(base[k], tuple):
            assert torch.equal(base[k], out1[k]), k
            continue
        a, b = [t.cpu().numpy() for t in base[k]], [t.cpu().numpy() for t in out1[k]]
        np.testing.assert_array_equal(a[-1], b[-1])
        for x, y in zip(a[:-1], b[:-1]):
            for cpi in range(x.shape[0]):
                m = min(int(a[-1][cpi, 0]), x.shape[1])
                assert x[cpi, :m].tobytes() == y[cpi, :m].tobytes(), k
    p = tr.Params(dt=proc.spec.P / proc.spec.radar["prf"], **TRACK)
    state = tr.new_state(4, p.max_tracks)
    plots = 0
    for out in (out1, out2):
        for part, kind in pairs:
            s = proc.TRACK_SLOTS[(part, kind)]
            est, _, count = (t.cpu().numpy() for t in out[(part, kind)])
            want = tr.run((state[0][s:s + 1], state[1][s:s + 1], state[2][s:s + 1]), est, count, p)
            _same(tuple(t.cpu().numpy() for t in out[(part, kind, "tracks")]), want, (part, kind))
            plots += int(want[3][:, tr.N_VALID].sum())
    _same(two_calls, state, "two calls")
    assert plots > 0 and state[2][:, 0].max() > 0 and state[2][:, 1].tolist() == [4, 4, 4, 4]
    # one call over both batches
    proc.reset_tracks()
    both = proc.process_dev(torch.cat([echo, echo.flip(0)]), 4, condense=condense, max_hits=512, track=TRACK)
    torch.cuda.synchronize()
    for part, kind in pairs:
        got = [t.cpu().numpy() for t in both[(part, kind, "tracks")]]
        parts = [[t.cpu().numpy() for t in o[(part, kind, "tracks")]] for o in (out1, out2)]
        _same(tuple(got), tuple(np.concatenate([q[i] for q in parts]) for i in range(4)), (part, kind, "one call"))
    _same(_state(proc._tracker), two_calls, "one call")
    proc.reset_tracks()
    assert not any(t.any() for t in proc._tracker.state())
    with pytest.raises(TypeError):
        proc.process_dev(echo, 4, track=dict(TRACK, gates=(1.0, 1.0)))
    with pytest.raises(TypeError):
        proc.process_dev(echo, 4, track=dict(alpha=(0.5, 0.5, 0.5)))
