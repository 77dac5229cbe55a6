"""Post-detection integration on the GPU (rsp_integrate_dev / rsp_binint_dev, csrc/rsp_integ.hip) against
the restatement tests/integ_ref.py, through the C ABI itself so that the window base, the pitch and the
state buffers are the test's own.

The kernel does the same fp32 additions in the same order, so nothing has a tolerance: d_out, d_neff,
d_hist and d_meta are compared byte for byte.  One allowance, for planes that hold NaN or opposite
infinities only: IEEE 754 leaves the sign and payload of a NaN result open (Inf + -Inf is 0x7fc00000 on
one machine and 0xffc00000 on another), so where the restatement's sum is a NaN the kernel's must be a
NaN, and every other cell must still have the same bytes.  The ring holds copies of the inputs and is
always compared byte for byte.

Every run puts sentinel bytes around d_out and d_hist and into the pitch's padding columns of d_out, and
starts from a ring filled with junk; all of that must come back untouched.
"""
import ctypes as C

import numpy as np
import pytest

import integ_ref as ir

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel elements on each side of d_out and d_hist
SENT = 0xA5

# (V, R, ld, column offset of the window, elements the whole input / output buffers are moved off
# their allocation's alignment)
SHAPES = [(5, 1, 1, 0, 0), (5, 7, 7, 0, 0), (64, 67, 67, 0, 0), (33, 130, 133, 3, 1), (16, 512, 574, 62, 0)]
SHAPE_IDS = ["5x1", "5x7", "64x67", "33x130of133odd", "16x512of574at62"]


@pytest.fixture(scope="module")
def rt():
    import torch
    from rsp import _capi as capi
    lib = capi.load_library()
    ctx = C.c_void_p()
    capi.check(lib.rsp_create(C.byref(ctx), 0, None), None)   # the CFAR-only kind
    yield capi, lib, ctx
    torch.cuda.synchronize()
    lib.rsp_destroy(ctx)


def _planes(rng, form, B, V, ld):
    """Full-pitch planes: noise magnitudes (sum) or sparse flags with a few bytes other than 1 (binary)."""
    if form == "sum":
        return np.abs(rng.standard_normal((B, V, ld))).astype(np.float32)
    f = (rng.random((B, V, ld)) < 0.25).astype(np.uint8)
    return f * rng.integers(1, 256, size=f.shape, dtype=np.uint8)


def _shift_table(n, V, R, rot=0):
    """Every kind of shift in one table: zero, +-1, small mixed signs, exactly +-(R-1) and +-R, beyond,
    and the ends of int32; rows and terms see different ones."""
    vals = [0, 1, -1, 2, -3, R - 1, -(R - 1), R, -R, R + 5, -(R + 7), 2 ** 31 - 1, -2 ** 31]
    return np.array([[vals[(v + 3 * i + rot) % len(vals)] for v in range(V)] for i in range(1, n)],
                    np.int64).astype(np.int32).reshape(n - 1, V)


def _gpu(rt, form, x, n, hist, meta, col0=0, R=None, off=0, shift=None, slot=None, m=0, spread=0, cuts=None,
         reset_at=None):
    """The calls on the device: x [B][V][ld] full-pitch planes whose window is columns col0 .. col0+R-1,
    hist / meta the state to start from (numpy, copied).  cuts: the batch as consecutive calls.
    reset_at: d_meta is zeroed before the call that starts at this CPI.  Returns (out window, neff,
    hist, meta) as numpy, after checking every sentinel."""
    import torch
    capi, lib, ctx = rt
    B, V, ld = x.shape
    R = ld - col0 if R is None else R
    dt = torch.float32 if form == "sum" else torch.uint8
    npdt = np.float32 if form == "sum" else np.uint8
    esz = 4 if form == "sum" else 1
    dev = "cuda:0"
    d_in = torch.zeros(B * V * ld + off, dtype=dt, device=dev)
    d_in[off:].copy_(torch.from_numpy(np.ascontiguousarray(x).reshape(-1)))
    d_out = torch.empty((B * V * ld + off + 2 * GUARD) * esz, dtype=torch.uint8, device=dev).fill_(SENT)
    d_hist = torch.empty((hist.size + 2 * GUARD) * esz, dtype=torch.uint8, device=dev).fill_(SENT)
    d_hist[GUARD * esz:(GUARD + hist.size) * esz].copy_(torch.from_numpy(hist.reshape(-1).view(np.uint8).copy()))
    d_meta = torch.from_numpy(meta.copy()).to(dev)
    d_neff = torch.full((B,), -7, dtype=torch.int32, device=dev)
    d_shift = None if shift is None else torch.from_numpy(np.ascontiguousarray(shift, dtype=np.int32)).to(dev)
    d_slot = None if slot is None else torch.from_numpy(np.ascontiguousarray(slot, dtype=np.int32)).to(dev)
    p = capi.rsp_integ_params()
    p.n, p.m, p.spread, p.reserved, p.ld, p.cpi_stride = n, m, spread, 0, ld, V * ld
    fn = lib.rsp_integrate_dev if form == "sum" else lib.rsp_binint_dev
    st = torch.cuda.current_stream().cuda_stream
    for a, b in zip((cuts or [0, B])[:-1], (cuts or [0, B])[1:]):
        if reset_at is not None and a == reset_at:
            d_meta.zero_()
        base = (off + a * V * ld + col0) * esz
        capi.check(fn(ctx, d_in.data_ptr() + base, V, R, b - a, C.byref(p),
                      d_shift.data_ptr() if d_shift is not None and d_shift.numel() else None,
                      d_slot.data_ptr() + 4 * a if d_slot is not None else None, meta.shape[0],
                      d_hist.data_ptr() + GUARD * esz if hist.size else None, d_meta.data_ptr(),
                      d_out.data_ptr() + GUARD * esz + base, d_neff.data_ptr() + 4 * a, C.c_void_p(st)), ctx)
    torch.cuda.synchronize()
    ob = d_out.cpu().numpy()
    hb = d_hist.cpu().numpy()
    assert (ob[:(GUARD + off) * esz] == SENT).all() and (ob[-GUARD * esz:] == SENT).all(), "d_out's guards were written"
    assert (hb[:GUARD * esz] == SENT).all() and (hb[-GUARD * esz:] == SENT).all(), "d_hist's guards were written"
    full = ob[(GUARD + off) * esz:-GUARD * esz].reshape(B, V, ld * esz)
    pad = np.ones(ld * esz, bool)
    pad[col0 * esz:(col0 + R) * esz] = False
    assert (full[:, :, pad] == SENT).all(), "columns of d_out outside the window were written"
    out = np.ascontiguousarray(full[:, :, ~pad]).view(npdt).reshape(B, V, R)
    hist_out = hb[GUARD * esz:len(hb) - GUARD * esz].view(npdt).reshape(hist.shape)
    return out, d_neff.cpu().numpy(), hist_out, d_meta.cpu().numpy()


def _ref(form, x, n, hist, meta, col0=0, R=None, shift=None, slot=None, m=0, spread=0, cuts=None, reset_at=None):
    B, V, ld = x.shape
    R = ld - col0 if R is None else R
    h, mt = hist.copy(), meta.copy()
    w = np.ascontiguousarray(x[:, :, col0:col0 + R])
    outs, neffs = [], []
    for a, b in zip((cuts or [0, B])[:-1], (cuts or [0, B])[1:]):
        if reset_at is not None and a == reset_at:
            mt[:] = 0
        o, ne = ir.run(w[a:b], n, h, mt, shift, None if slot is None else slot[a:b], None if form == "sum" else m, spread)
        outs.append(o)
        neffs.append(ne)
    return np.concatenate(outs), np.concatenate(neffs), h, mt


def _same(got, want, what, nan_open=False):
    for name, g, w in zip(("out", "neff", "hist", "meta"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if nan_open and name == "out":
            wn = np.isnan(w)
            assert (np.isnan(g) == wn).all(), (what, "NaN cells differ")
            g, w = np.where(wn, np.float32(0), g), np.where(wn, np.float32(0), w)
        if g.tobytes() != w.tobytes():
            iv = {4: np.uint32, 1: np.uint8}[g.dtype.itemsize]
            bad = np.argwhere(g.view(iv) != w.view(iv))
            raise AssertionError("%s: %s differs at %d places, first %s: got %r, want %r"
                                 % (what, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def _both(rt, form, x, n, slots=1, junk=5, **kw):
    V = x.shape[1]
    R = kw.get("R") or x.shape[2] - kw.get("col0", 0)
    hist, meta = ir.new_state(slots, n, V, R, x.dtype, junk=junk)
    ref_kw = {k: v for k, v in kw.items() if k != "off"}
    return _gpu(rt, form, x, n, hist, meta, **kw), _ref(form, x, n, hist, meta, **ref_kw)


# ---------------------------------------------------------------- shapes x n, every kind of shift
@pytest.mark.parametrize("n", [1, 2, 3, 4, 8, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_sum_matches_the_restatement(rt, shape, n):
    V, R, ld, col0, off = shape
    B = n + 3
    x = _planes(np.random.default_rng(100 * n + V), "sum", B, V, ld)
    got, want = _both(rt, "sum", x, n, col0=col0, R=R, off=off, shift=_shift_table(n, V, R, rot=n))
    _same(got, want, "sum %s n=%d" % (shape, n))
    assert got[1].tolist() == [min(n, b + 1) for b in range(B)]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 8, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_binary_matches_the_restatement(rt, shape, n):
    V, R, ld, col0, off = shape
    B = n + 3
    x = _planes(np.random.default_rng(200 * n + V), "binary", B, V, ld)
    for m in sorted({1, (n + 1) // 2, n}):          # 1, one between, n
        spread = (m + n) % 3
        got, want = _both(rt, "binary", x, n, col0=col0, R=R, off=off, shift=_shift_table(n, V, R, rot=m), m=m,
                          spread=spread)
        _same(got, want, "binary %s n=%d m=%d spread=%d" % (shape, n, m, spread))
        if m > 1:
            assert not got[0][:m - 1].any()         # strict: nothing before the slot's m-th CPI


SHIFT_KINDS = ["null", "zero", "+1", "-1", "+(R-1)", "-(R-1)", "+R", "-R", "beyond"]


@pytest.mark.parametrize("form", ["sum", "binary"])
@pytest.mark.parametrize("kind", SHIFT_KINDS)
def test_uniform_shifts(rt, form, kind):
    V, R, ld, col0, off = SHAPES[3]
    n, B = 4, 6
    val = {"null": None, "zero": 0, "+1": 1, "-1": -1, "+(R-1)": R - 1, "-(R-1)": -(R - 1), "+R": R, "-R": -R,
           "beyond": 3 * R + 1}[kind]
    # term i moves by i * val: the first term sits exactly on the stated value
    shift = None if val is None else (np.arange(1, n)[:, None] * np.full((1, V), val)).astype(np.int32)
    x = _planes(np.random.default_rng(11), form, B, V, ld)
    kw = dict(m=2, spread=1) if form == "binary" else {}
    got, want = _both(rt, form, x, n, col0=col0, R=R, off=off, shift=shift, **kw)
    _same(got, want, "%s shift %s" % (form, kind))
    if form == "sum" and kind in ("+R", "-R", "beyond"):
        w = x[:, :, col0:col0 + R]
        assert got[0].tobytes() == w.tobytes()      # every term vanished: x + (+0) = x for magnitudes
    if kind in ("null", "zero"):
        z = _gpu(rt, form, x, n, *ir.new_state(1, n, V, R, x.dtype, junk=5), col0=col0, R=R, off=off,
                 shift=None if kind == "zero" else np.zeros((n - 1, V), np.int32), **kw)
        _same(z, got, "NULL shifts against zeros")


# ---------------------------------------------------------------- the point of it
def test_a_walking_target_piles_up_in_one_cell(rt):
    V, R, n = 64, 67, 4
    rng = np.random.default_rng(3)
    x = (0.01 * np.abs(rng.standard_normal((n, V, R)))).astype(np.float32)
    shift = _shift_table(n, V, R)
    shift[:, 20] = [2, 4, 6]           # row 20 walks two columns per CPI
    shift[:, 41] = [-3, -6, -9]        # row 41 three the other way
    amp = np.array([10.0, 11.5, 9.25, 12.125], np.float32)
    for b in range(n):
        x[b, 20, 30 + 2 * b] = amp[b]
        x[b, 41, 50 - 3 * b] = amp[b]
    got, want = _both(rt, "sum", x, n, shift=shift)
    _same(got, want, "walking target")
    last = got[0][n - 1]
    total = np.float32(np.float32(np.float32(amp[3] + amp[2]) + amp[1]) + amp[0])   # x_0 + x_1 + x_2 + x_3
    for v, c in ((20, 36), (41, 41)):
        assert last[v, c] == total
        row = last[v].copy()
        row[c] = 0
        assert row.max() < 1.0          # one cell holds the sum, nothing of it is left beside it
    # without the shifts the same target smears over n cells
    plain, _ = _both(rt, "sum", x, n)
    assert (plain[0][n - 1][20] > 5.0).sum() == n


def test_nan_inf_and_minus_zero(rt):
    V, R, ld, col0, off = SHAPES[3]
    n, B = 4, 9
    rng = np.random.default_rng(17)
    x = _planes(rng, "sum", B, V, ld)
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], np.float32)
    pick = rng.random(x.shape) < 0.08
    x[pick] = specials[rng.integers(0, len(specials), size=int(pick.sum()))]
    x[:, 5, :] = -0.0                   # a row of -0: stays -0 alone, turns +0 when a term from outside is added
    shift = _shift_table(n, V, R)
    got, want = _both(rt, "sum", x, n, col0=col0, R=R, off=off, shift=shift)
    _same(got, want, "specials", nan_open=True)
    assert np.isnan(want[0]).any() and np.isinf(want[0]).any()
    assert np.signbit(got[0][0, 5]).all()
    z = got[0][:, 5]
    assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()


# ---------------------------------------------------------------- slots, batch lengths, reset
def _slot_case(form, seed, B, V, ld, slots, pattern):
    x = _planes(np.random.default_rng(seed), form, B, V, ld)
    slot = np.array([pattern[b % len(pattern)] for b in range(B)], np.int32)
    return x, slot


@pytest.mark.parametrize("form", ["sum", "binary"])
@pytest.mark.parametrize("n,B", [(8, 2), (3, 40), (4, 13), (16, 21)], ids=["short", "long", "mid", "n16"])
def test_slots_and_split_invariance(rt, form, n, B):
    V, R, ld, col0, off = 33, 130, 133, 3, 1
    slots = 3
    # three slots interleaved, and -1 and `slots` (both out of range) inside the batch
    x, slot = _slot_case(form, 31 + n, B, V, ld, slots, [0, 1, 0, 2, -1, 1, 0, slots, 2, 0])
    kw = dict(col0=col0, R=R, off=off, shift=_shift_table(n, V, R), slot=slot, slots=slots)
    if form == "binary":
        kw.update(m=2, spread=1)
    whole, want = _both(rt, form, x, n, **kw)
    _same(whole, want, "slots, one batch")
    out_of_range = (slot < 0) | (slot >= slots)
    assert (whole[1][out_of_range] == 1).all()
    again, _ = _both(rt, form, x, n, **kw)
    _same(again, whole, "the same call twice")
    for cuts in (list(range(B + 1)), [0, min(3, B), B] if B > 3 else [0, 1, B]):
        got, _ = _both(rt, form, x, n, cuts=cuts, **kw)
        _same(got, whole, "split %s" % (cuts[:4],))


@pytest.mark.parametrize("form", ["sum", "binary"])
def test_null_slot_is_slot_zero(rt, form):
    V, R, n, B = 5, 7, 4, 9
    x = _planes(np.random.default_rng(41), form, B, V, R)
    kw = dict(m=3, spread=2) if form == "binary" else {}
    a, want = _both(rt, form, x, n, slots=2, shift=_shift_table(n, V, R), **kw)
    _same(a, want, "NULL slot")
    b, _ = _both(rt, form, x, n, slots=2, shift=_shift_table(n, V, R), slot=np.zeros(B, np.int32), **kw)
    _same(b, a, "NULL slot against zeros")
    assert a[3].tolist() == [[B, 0], [0, 0]]


@pytest.mark.parametrize("form", ["sum", "binary"])
def test_reset_in_mid_sequence(rt, form):
    V, R, n, B = 64, 67, 4, 12
    x = _planes(np.random.default_rng(43), form, B, V, R)
    base = dict(m=2, spread=0) if form == "binary" else {}
    base.update(shift=_shift_table(n, V, R))
    got, want = _both(rt, form, x, n, cuts=[0, 7, B], reset_at=7, **base)
    _same(got, want, "reset")
    assert got[1].tolist() == [1, 2, 3, 4, 4, 4, 4, 1, 2, 3, 4, 4]
    # the CPIs after the reset come out as a fresh integrator gives them, whatever the ring still holds
    fresh, _ = _both(rt, form, x[7:], n, junk=77, **base)
    assert got[0][7:].tobytes() == fresh[0].tobytes()


def test_python_wrapper_windows_and_state(rt):
    import torch
    from rsp.integrate import Integrator, walk_shifts
    V, Rp, n, B = 16, 574, 4, 6
    x = _planes(np.random.default_rng(47), "sum", B, V, Rp)
    shift = walk_shifts(np.linspace(-400.0, 400.0, V), 0.08, 12.0, n)
    integ = Integrator(0, n=n, m=2, spread=1)
    try:
        for cols in ((0, 62), (62, 574)):
            integ.reset()
            out = torch.full((B, V, Rp), 7.0, dtype=torch.float32, device="cuda:0")
            o, ne = integ.sum_dev(torch.from_numpy(x).cuda(), shift=shift, cols=cols, out=out)
            torch.cuda.synchronize()
            lo, hi = cols
            hist, meta = ir.new_state(1, n, V, hi - lo, np.float32)
            want, wne = ir.run(np.ascontiguousarray(x[:, :, lo:hi]), n, hist, meta, shift=shift)
            g = o.cpu().numpy()
            assert g[:, :, lo:hi].tobytes() == want.tobytes() and ne.cpu().numpy().tolist() == wne.tolist()
            assert (np.delete(g, np.s_[lo:hi], axis=2) == 7.0).all()
            assert integ.hist.cpu().numpy().tobytes() == hist.tobytes() and integ.meta.cpu().numpy().tolist() == meta.tolist()
        with pytest.raises(ValueError):
            integ.sum_dev(torch.from_numpy(x).cuda(), cols=(0, 62))   # another window without a reset
        integ.reset()
        f = _planes(np.random.default_rng(48), "binary", B, V, Rp)
        o, _ = integ.count_dev(torch.from_numpy(f).cuda(), shift=shift)
        torch.cuda.synchronize()
        hist, meta = ir.new_state(1, n, V, Rp, np.uint8)
        want, _ = ir.run(f, n, hist, meta, shift=shift, m=2, spread=1)
        assert o.cpu().numpy().tobytes() == want.tobytes()
    finally:
        integ.close()
