"""The hit list and the measurement (csrc/rsp_measure.hip: hits_kernel, measure_kernel<1..4>)
swept over the designed cases of tests/measure_cases.py against the fp64 oracle
(oracle/measure_ref.py), through the C entry point on window buffers.

Bar: bit-exact, nothing excluded.  Both counts equal the oracle's over all hits (not only the first
max_hits), the cells are equal, and every estimate the oracle gives a number for is compared as a
64-bit word (which tells -0 from +0, and +inf from -inf); where the oracle's value is NaN only
NaN-ness is compared, because the sign and payload of a NaN differ between the host and the GPU.
The outputs sit inside arrays with 16 sentinel elements either side, the slots at or past
min(count, max_hits) hold sentinels too, and everything round the input windows holds 3e30
amplitudes and set flags: a write or a read outside shows.  Each case also runs twice (same
bytes), with CPI 1 alone (the bytes it had in the batch), without d_cells and with max_hits = 0.

tests/test_measure_cases_cpu.py shows, on the CPU and against the oracle alone, that each scene
holds what its row is for; tests/test_measure_cpu.py runs the kernel's arithmetic header on the
host against the oracle.

Not covered here: the banded hit lists (band_count / band_scan / band_list kernels).  They are
compiled into the library but unreachable in it (measure_bands() returns 1 unless the library is
built with -DRSP_DEV_MEASURE_BANDS), so every case here, and every other measurement test, runs
hits_kernel.
"""
import ctypes as C

import numpy as np
import pytest

import condense_ref
import measure_cases as mc
import measure_ref as mr

pytestmark = pytest.mark.gpu

GUARD = 16
SENT_I64 = -0x0123456789ABCDEF          # as a float64 word: a finite number no estimate equals
SENT_I32 = -7777
IDS = [c.id for c in mc.CASES]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from rsp.condense import Condense
    from rsp.measure import Measure
    m, c = Measure(0), Condense(0)
    yield m, c
    m.close()
    c.close()


def _params(meas, c, **over):
    p = meas.params(c.e, mc.FIXED["delta_r"], c.interp[0], mc.FIXED["delta_v"], c.interp[1], mc.FIXED["k_value"],
                    mc.FIXED["beam_pos_num"], mc.FIXED["beam_angle_step"], mc.FIXED["ele_comp"],
                    mc.FIXED["ele_sys_err"], c.M0)
    p.ld, p.cpi_stride = c.ld, c.cs
    for k, v in over.items():
        setattr(p, k, v)
    return p


class _Dev:
    """A scene's buffers on the device."""

    def __init__(self, sc):
        import torch
        self.host = sc.buffers()
        self.s, self.d, self.f = (torch.from_numpy(x).cuda() for x in self.host)
        self.rs = torch.from_numpy(sc.r_scale).cuda()
        self.vs = torch.from_numpy(sc.v_scale).cuda()

    def unchanged(self):
        for h, t in zip(self.host, (self.s, self.d, self.f)):
            assert h.tobytes() == t.cpu().numpy().tobytes(), "an input plane was written"


def _call(meas, c, dev, first_cpi=0, n=mc.BATCH, max_hits=None, with_cells=True, with_est=True, params=None):
    """rsp_motion_measure_dev on CPIs first_cpi.. of the window buffers, the outputs inside guarded,
    sentinel-filled arrays.  Returns (status, est words int64 [n][mh][3], cells [n][mh][2], count [n][2])."""
    import torch
    mh = c.max_hits if max_hits is None else max_hits
    est = torch.full((GUARD + n * mh * 3 + GUARD,), SENT_I64, dtype=torch.int64, device="cuda")
    cells = torch.full((GUARD + n * mh * 2 + GUARD,), SENT_I32, dtype=torch.int32, device="cuda")
    count = torch.full((GUARD + n * 2 + GUARD,), SENT_I32, dtype=torch.int32, device="cuda")
    p = _params(meas, c) if params is None else params
    off = mc.GUARD + first_cpi * c.cs + c.col0
    st = torch.cuda.current_stream().cuda_stream
    rc = meas.lib.rsp_motion_measure_dev(
        meas.ctx, dev.s.data_ptr() + 4 * off, dev.d.data_ptr() + 4 * off, dev.f.data_ptr() + off, c.V, c.R, n, C.byref(p),
        dev.rs.data_ptr(), dev.vs.data_ptr(), mh, est.data_ptr() + 8 * GUARD if with_est else None,
        cells.data_ptr() + 4 * GUARD if with_cells else None, count.data_ptr() + 4 * GUARD, C.c_void_p(st))
    torch.cuda.synchronize()
    est, cells, count = est.cpu().numpy(), cells.cpu().numpy(), count.cpu().numpy()
    assert (est[:GUARD] == SENT_I64).all() and (est[-GUARD:] == SENT_I64).all(), "written outside d_est"
    assert (cells[:GUARD] == SENT_I32).all() and (cells[-GUARD:] == SENT_I32).all(), "written outside d_cells"
    assert (count[:GUARD] == SENT_I32).all() and (count[-GUARD:] == SENT_I32).all(), "written outside d_count"
    return rc, est[GUARD:-GUARD].reshape(n, mh, 3), cells[GUARD:-GUARD].reshape(n, mh, 2), count[GUARD:-GUARD].reshape(n, 2)


def _compare(c, est, cells, count, oracle, cpis):
    """The bit-exact bar for the CPIs `cpis` of the oracle, output row i against cpis[i]."""
    mh = est.shape[1]
    for i, b in enumerate(cpis):
        want, hc = oracle[b]
        n = len(hc)
        failed = np.isnan(want[:, 0])
        assert count[i, 0] == n, (c.id, b, "hits")
        assert count[i, 1] == int(failed.sum()), (c.id, b, "failed hits, over all hits")
        w = min(n, mh)
        np.testing.assert_array_equal(cells[i, :w], hc[:w], err_msg="%s cpi %d cells" % (c.id, b))
        got = est[i, :w].view(np.float64)
        want_w = np.ascontiguousarray(want[:w])
        nan = np.isnan(want_w)
        assert np.array_equal(np.isnan(got), nan), (c.id, b, "NaN-ness")
        bad = (est[i, :w].view(np.uint64) != want_w.view(np.uint64)) & ~nan
        assert not bad.any(), (c.id, b, np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want_w[bad][:4].tolist())
        # a failed hit is NaN in all three columns; a measured one may be non-finite in its elevation only
        assert nan[failed[:w]].all() and np.isfinite(got[~failed[:w]][:, :2]).all()
        assert (est[i, w:] == SENT_I64).all(), (c.id, b, "d_est written at or past min(count, max_hits)")
        assert (cells[i, w:] == SENT_I32).all(), (c.id, b, "d_cells written at or past min(count, max_hits)")


@pytest.mark.parametrize("c", mc.CASES, ids=IDS)
def test_case(gpu, c):
    from rsp import _capi as capi
    meas, _ = gpu
    sc = mc.scene(c)
    oracle = sc.oracle()
    dev = _Dev(sc)
    # the plan the row names, from the call's own arguments
    out = capi.rsp_measure_plan_t()
    p = _params(meas, c)
    capi.check(meas.lib.rsp_measure_plan(meas.ctx, dev.f.data_ptr() + mc.GUARD + c.col0, c.V, c.R, mc.BATCH, C.byref(p),
                                         C.byref(out)), meas.ctx)
    assert dict(wide=bool(out.wide), G=out.groups, S=out.slices, rows=out.rows, q=out.q, passes=out.passes) == c.plan
    assert out.bands == 1 and out.cw == (16 if c.plan["wide"] else 1)
    # the batch against the oracle
    rc, est, cells, count = _call(meas, c, dev)
    assert rc == 0
    _compare(c, est, cells, count, oracle, range(mc.BATCH))
    # a second run gives the same bytes
    rc, est2, cells2, count2 = _call(meas, c, dev)
    assert rc == 0 and est2.tobytes() == est.tobytes() and cells2.tobytes() == cells.tobytes() and \
        count2.tobytes() == count.tobytes()
    # CPI 1 alone gives the bytes it had in the batch
    rc, est1, cells1, count1 = _call(meas, c, dev, first_cpi=1, n=1)
    assert rc == 0 and est1[0].tobytes() == est[1].tobytes() and cells1[0].tobytes() == cells[1].tobytes() and \
        count1[0].tobytes() == count[1].tobytes()
    # d_cells = NULL: the same d_est and d_count
    rc, est3, cells3, count3 = _call(meas, c, dev, with_cells=False)
    assert rc == 0 and est3.tobytes() == est.tobytes() and count3.tobytes() == count.tobytes()
    assert (cells3 == SENT_I32).all()
    # max_hits = 0 with d_est = NULL: the same d_count
    rc, _, _, count4 = _call(meas, c, dev, max_hits=0, with_cells=False, with_est=False)
    assert rc == 0 and count4.tobytes() == count.tobytes()
    dev.unchanged()


@pytest.mark.parametrize("cid", ["b-2pass", "w-2pass"])
def test_condense_then_measure_across_two_passes(gpu, cid):
    """rsp_condense_dev (gap 1, 1) on the two-pass shapes, then rsp_motion_measure_dev on its peak
    plane: hit i of the measurement is plot i of d_plots, and both are condense_ref followed by the
    oracle.  The plot list is hits_kernel's (launch_hit_list), so this is where its multi-pass order
    reaches the tracker's input."""
    import torch
    from rsp import _capi as capi
    meas, cond = gpu
    c = mc.BY_ID[cid]
    sc = mc.scene(c)
    V, R, B = c.V, c.R, mc.BATCH
    per_pass = c.plan["G"] * (16 if c.plan["wide"] else 1)
    refs = [condense_ref.condense(sc.s[b], sc.f[b], gap=(1, 1)) for b in range(B)]
    for rp, rpl, (n_plots, n_hits) in refs:
        assert 0 < n_plots <= n_hits and set((rpl[:, 1] // per_pass).tolist()) == {0, 1}   # plots in both passes
    mh = max(r[2][0] for r in refs) + 3
    d_s, d_d, d_f = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (sc.s, sc.d, sc.f))
    d_peak = torch.full((B, V, R), 0xAB, dtype=torch.uint8, device="cuda")
    d_plots = torch.full((B, mh, 8), SENT_I32, dtype=torch.int32, device="cuda")
    d_pc = torch.full((B, 2), SENT_I32, dtype=torch.int32, device="cuda")
    cp = capi.rsp_condense_params()
    cp.gap_v, cp.gap_r, cp.wrap_v, cp.ld, cp.cpi_stride = 1, 1, 0, R, V * R
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi.check(cond.lib.rsp_condense_dev(cond.ctx, d_s.data_ptr(), d_f.data_ptr(), V, R, B, C.byref(cp), d_peak.data_ptr(),
                                         mh, d_plots.data_ptr(), d_pc.data_ptr(), st), cond.ctx)
    # the plan of the list condense made: the peak plane's address with the window's geometry
    out = capi.rsp_measure_plan_t()
    p = _params(meas, c, ld=R, cpi_stride=V * R)
    capi.check(meas.lib.rsp_measure_plan(meas.ctx, d_peak.data_ptr(), V, R, B, C.byref(p), C.byref(out)), meas.ctx)
    assert bool(out.wide) == c.plan["wide"] and out.passes == 2
    d_est = torch.full((B, mh, 3), SENT_I64, dtype=torch.int64, device="cuda")
    d_cells = torch.full((B, mh, 2), SENT_I32, dtype=torch.int32, device="cuda")
    d_mc = torch.full((B, 2), SENT_I32, dtype=torch.int32, device="cuda")
    d_rs, d_vs = torch.from_numpy(sc.r_scale).cuda(), torch.from_numpy(sc.v_scale).cuda()
    capi.check(meas.lib.rsp_motion_measure_dev(meas.ctx, d_s.data_ptr(), d_d.data_ptr(), d_peak.data_ptr(), V, R, B,
                                               C.byref(p), d_rs.data_ptr(), d_vs.data_ptr(), mh, d_est.data_ptr(),
                                               d_cells.data_ptr(), d_mc.data_ptr(), st), meas.ctx)
    torch.cuda.synchronize()
    peak, plots, pc = d_peak.cpu().numpy(), d_plots.cpu().numpy(), d_pc.cpu().numpy()
    est, cells, count = d_est.cpu().numpy(), d_cells.cpu().numpy(), d_mc.cpu().numpy()
    oracle = []
    for b, (rp, rpl, (n_plots, n_hits)) in enumerate(refs):
        assert tuple(pc[b]) == (n_plots, n_hits)
        np.testing.assert_array_equal(peak[b], rp)
        np.testing.assert_array_equal(plots[b, :n_plots], rpl)
        assert (plots[b, n_plots:] == SENT_I32).all()
        np.testing.assert_array_equal(cells[b, :n_plots], plots[b, :n_plots, :2])      # hit i is plot i
        re, ve, el, hc = mr.motion_para_measure(sc.s[b].astype(np.float64), sc.d[b].astype(np.float64), rp,
                                                on_error="nan", **sc.kw)
        oracle.append((np.stack([re, ve, el], axis=1).reshape(-1, 3), hc))
        np.testing.assert_array_equal(hc, rpl[:, :2])
    _compare(c, est, cells, count, oracle, range(B))


def test_refusals_leave_the_outputs_untouched(gpu):
    """Every documented refusal of rsp_motion_measure_dev on a live context: its status, and
    sentinel-filled d_est / d_cells / d_count untouched.  rsp_measure_plan answers the same for what
    it shares with the call (the shape, the parameters, mp and d_flag)."""
    import torch
    from rsp import _capi as capi
    meas, _ = gpu
    ARG, UNSUP = capi.RSP_ERR_ARG, capi.RSP_ERR_UNSUPPORTED
    c = mc.BY_ID["b-cs"]
    dev = _Dev(mc.scene(c))
    V, R, B, mh = c.V, c.R, mc.BATCH, 16
    off = mc.GUARD + c.col0
    est = torch.full((B * mh * 3,), SENT_I64, dtype=torch.int64, device="cuda")
    cells = torch.full((B * mh * 2,), SENT_I32, dtype=torch.int32, device="cuda")
    count = torch.full((B * 2,), SENT_I32, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(want, shared=True, **kw):
        a = dict(s=dev.s.data_ptr() + 4 * off, d=dev.d.data_ptr() + 4 * off, f=dev.f.data_ptr() + off, V=V, R=R, B=B,
                 rs=dev.rs.data_ptr(), vs=dev.vs.data_ptr(), mh=mh, est=est.data_ptr(), cells=cells.data_ptr(),
                 count=count.data_ptr(), p={})
        a.update(kw)
        p = None if a["p"] is None else _params(meas, c, **a["p"])
        ref = None if p is None else C.byref(p)
        rc = meas.lib.rsp_motion_measure_dev(meas.ctx, a["s"], a["d"], a["f"], a["V"], a["R"], a["B"], ref, a["rs"], a["vs"],
                                             a["mh"], a["est"], a["cells"], a["count"], st)
        assert rc == want, (kw, rc, meas.lib.rsp_last_error(meas.ctx))
        if shared:
            out = capi.rsp_measure_plan_t()
            assert meas.lib.rsp_measure_plan(meas.ctx, a["f"], a["V"], a["R"], a["B"], ref, C.byref(out)) == want, kw
        torch.cuda.synchronize()
        assert (est == SENT_I64).all() and (cells == SENT_I32).all() and (count == SENT_I32).all(), kw

    call(ARG, R=4)                                               # R < 2e+1 (e = 2)
    call(ARG, p=dict(mtd0_num=18))                               # V - 2*M0 - 1 = 3 < 2e+1
    call(ARG, p=dict(mtd0_num=-1))
    call(UNSUP, p=dict(extra_dots=0))
    call(UNSUP, p=dict(extra_dots=5))
    for k in ("r_interp", "v_interp"):
        call(ARG, p={k: 0})
        call(ARG, p={k: 65})
    call(ARG, p=dict(ld=R - 1))
    call(ARG, p=dict(cpi_stride=(V - 1) * c.ld + R - 1))
    call(ARG, V=0)
    call(ARG, B=-1)
    call(ARG, p=None)
    call(ARG, f=None)
    for k in ("s", "d", "rs", "vs", "count"):
        call(ARG, shared=False, **{k: None})
    call(ARG, shared=False, est=None)                            # max_hits > 0 needs d_est
    call(ARG, shared=False, mh=-1)
    assert meas.lib.rsp_motion_measure_dev(None, dev.s.data_ptr(), dev.d.data_ptr(), dev.f.data_ptr(), V, R, B, None, None,
                                           None, 0, None, None, None, st) == ARG
    # the edge of each bound is accepted (and an empty batch writes nothing)
    call(0, B=0, p=dict(extra_dots=2, mtd0_num=17))              # V - 2*M0 - 1 == 2e+1
    dev.unchanged()
