"""Post-detection integration, CPU side: the restatement tests/integ_ref.py against hand values and
against itself under batch splits, the fp32 sum against the fp64 sum within the bound of sequential
summation, walk_shifts against hand values, and the C ABI's refusals (rsp_integrate_dev / rsp_binint_dev
check everything they can before they look at the context).
"""
import ctypes as C

import numpy as np
import pytest

import integ_ref as ir


def _planes(rng, B, V, R):
    return np.abs(rng.standard_normal((B, V, R))).astype(np.float32)


# ---------------------------------------------------------------- the restatement by hand
def test_sum_by_hand_ring_and_meta():
    x = np.arange(1, 6, dtype=np.float32).reshape(5, 1, 1) * np.ones((5, 1, 3), np.float32)
    hist, meta = ir.new_state(1, 3, 1, 3, np.float32)
    out, neff = ir.run(x, 3, hist, meta)
    assert neff.tolist() == [1, 2, 3, 3, 3]
    assert out[:, 0, 0].tolist() == [1.0, 3.0, 6.0, 9.0, 12.0]
    # CPI k goes to entry k mod 2: the ring holds CPIs 4 (entry 0, value 5) and 3 (entry 1, value 4)
    assert hist[0, :, 0, 0].tolist() == [5.0, 4.0] and meta.tolist() == [[5, 0]]


def test_shift_moves_right_and_nothing_wraps():
    x = np.zeros((2, 2, 4), np.float32)
    x[0, 0, 1] = 2.0
    x[0, 1, 3] = 7.0
    shift = np.array([[1, 1]], np.int32)
    hist, meta = ir.new_state(1, 2, 2, 4, np.float32)
    out, _ = ir.run(x, 2, hist, meta, shift=shift)
    assert out[1].tolist() == [[0.0, 0.0, 2.0, 0.0], [0.0, 0.0, 0.0, 0.0]]   # the 7 left the window


def test_minus_zero_gets_plus_zero_added_only_from_a_past_plane():
    x = np.full((2, 1, 2), -0.0, np.float32)
    hist, meta = ir.new_state(1, 2, 1, 2, np.float32)
    out, _ = ir.run(x, 2, hist, meta, shift=np.array([[5]], np.int32))
    assert np.signbit(out[0]).all()            # n_eff = 1: the CPI itself
    assert not np.signbit(out[1]).any()        # -0 + (+0 from outside the window) = +0


def test_binary_strict_and_spread():
    f = np.zeros((3, 1, 6), np.uint8)
    f[0, 0, 1] = 1
    f[1, 0, 3] = 9     # any nonzero byte is a hit
    f[2, 0, 4] = 1
    shift = np.array([[1], [2]], np.int32)
    hist, meta = ir.new_state(1, 3, 1, 6, np.uint8)
    out, neff = ir.run(f, 3, hist, meta, shift=shift, m=3, spread=1)
    # CPI 2 at column 4: itself; CPI 1 walked 1: source 3 hit; CPI 0 walked 2: source 2, spread reaches 1
    assert out[2, 0].tolist() == [0, 0, 0, 0, 1, 0] and not out[:2].any()
    hist, meta = ir.new_state(1, 3, 1, 6, np.uint8)
    out, _ = ir.run(f, 3, hist, meta, shift=shift, m=3, spread=0)
    assert not out.any()
    assert hist[0, 1, 0].tolist() == [0, 0, 0, 9, 0, 0]   # the ring keeps the input bytes


def test_spread_reaches_into_the_window_from_outside():
    f = np.zeros((2, 1, 4), np.uint8)
    f[0, 0, 0] = 1
    hist, meta = ir.new_state(1, 2, 1, 4, np.uint8)
    # column 0 now: source column 0 - 1 = -1 is outside, its spread neighbour 0 is inside and set
    out, _ = ir.run(f, 2, hist, meta, shift=np.array([[1]], np.int32), m=1, spread=1)
    assert out[1, 0].tolist() == [1, 1, 1, 0]


# ---------------------------------------------------------------- split invariance
@pytest.mark.parametrize("form", ["sum", "binary"])
@pytest.mark.parametrize("n", [1, 2, 4])
def test_restatement_is_split_invariant(form, n):
    rng = np.random.default_rng(7 + n)
    B, V, R, slots = 11, 3, 9, 3
    if form == "sum":
        x, kw, dt = _planes(rng, B, V, R), {}, np.float32
    else:
        x, kw, dt = (rng.random((B, V, R)) < 0.3).astype(np.uint8), dict(m=max(1, n - 1), spread=1), np.uint8
    shift = rng.integers(-3, 4, size=(n - 1, V)).astype(np.int32)
    slot = np.array([0, 1, 0, 2, -1, 1, 0, 3, 0, 1, 0], np.int32)   # interleaved, -1 and `slots` out of range
    res = []
    for cuts in ([0, B], list(range(B + 1)), [0, 3, B]):
        hist, meta = ir.new_state(slots, n, V, R, dt, junk=99)
        out, neff = ir.split_run(x, n, hist, meta, cuts, shift=shift, slot=slot, **kw)
        res.append((out, neff, hist, meta))
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert a.tobytes() == b.tobytes()
    assert res[0][3][:, 0].tolist() == [5, 3, 1] and res[0][1][[4, 7]].tolist() == [1, 1]


# ---------------------------------------------------------------- fp32 against fp64
@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_fp32_sum_within_the_sequential_summation_bound(n):
    # |fl(sum) - sum| <= gamma_{n-1} * sum |x_i| for n-1 sequential additions, gamma_k = k u / (1 - k u),
    # u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4); the planes are >= 0
    rng = np.random.default_rng(n)
    B, V, R = n + 3, 16, 257
    x = _planes(rng, B, V, R)
    hist, meta = ir.new_state(1, n, V, R, np.float32)
    out, neff = ir.run(x, n, hist, meta)
    u = 2.0 ** -24
    gamma = (n - 1) * u / (1.0 - (n - 1) * u)
    worst = 0.0
    for b in range(B):
        exact = x[max(0, b - n + 1):b + 1].astype(np.float64).sum(axis=0)
        err = np.abs(out[b].astype(np.float64) - exact)
        assert (err <= gamma * exact).all()
        if b >= n - 1:
            worst = max(worst, float((err / (gamma * exact)).max()))
    assert 0.0 < worst <= 1.0


# ---------------------------------------------------------------- walk_shifts
def test_walk_shifts_hand_values():
    from rsp.integrate import walk_shifts
    # 0.5, 1.5, 2.5 cells per CPI: half-way cases round to even
    s = walk_shifts([0.5, 1.5, 2.5, -0.5, -1.5], 1.0, 1.0, 3)
    assert s.dtype == np.int32 and s.shape == (2, 5)
    assert s.tolist() == [[0, 2, 2, 0, -2], [1, 3, 5, -1, -3]]
    assert walk_shifts([0.5, 1.5, 2.5, -0.5, -1.5], 1.0, 1.0, 3, rate_sign=-1.0).tolist() == [[0, -2, -2, 0, 2],
                                                                                            [-1, -3, -5, 1, 3]]
    assert walk_shifts([1.0, 2.0], 1.0, 1.0, 1).shape == (0, 2)


def test_walk_shifts_dmx_numbers():
    from rsp.integrate import walk_shifts
    dt = 1536 * 52.08e-6                 # 79.99 ms
    delta_r = 299792458.0 / (2 * 12.5e6)   # 11.99 m
    # 150 m/s: 150 * 0.07999488 / 11.9917 = 1.0006 cells per CPI; 75 m/s: 0.5003; 37 m/s: 0.2468
    s = walk_shifts([150.0, -150.0, 75.0, 37.0, 0.0], dt, delta_r, 4)
    assert s.tolist() == [[1, -1, 1, 0, 0], [2, -2, 1, 0, 0], [3, -3, 2, 1, 0]]
    assert walk_shifts([150.0], dt, delta_r, 4, rate_sign=-1.0).tolist() == [[-1], [-2], [-3]]


# ---------------------------------------------------------------- the C ABI's refusals
def _lib():
    from rsp import _capi as capi
    return capi, capi.load_library()


def _call(lib, capi, form="sum", V=4, R=8, batch=2, d_in=1 << 40, d_hist=2 << 40, d_meta=3 << 40, d_out=4 << 40,
          slots=1, params=True, **kw):
    p = capi.rsp_integ_params()
    p.n, p.m, p.spread = 4, (0 if form == "sum" else 2), 0
    for k, v in kw.items():
        setattr(p, k, v)
    fn = lib.rsp_integrate_dev if form == "sum" else lib.rsp_binint_dev
    rc = fn(None, d_in, V, R, batch, C.byref(p) if params else None, None, None, slots, d_hist, d_meta, d_out, None, None)
    return rc, (lib.rsp_last_error(None) or b"").decode()


BAD = [
    ("null params", dict(params=False)),
    ("null d_in", dict(d_in=None)),
    ("null d_meta", dict(d_meta=None)),
    ("null d_out", dict(d_out=None)),
    ("null d_hist", dict(d_hist=None)),
    ("n = 0", dict(n=0)),
    ("n = 17", dict(n=17)),
    ("sum with m", dict(m=1)),
    ("sum with spread", dict(spread=1)),
    ("binary m = 0", dict(form="binary", m=0)),
    ("binary m > n", dict(form="binary", m=5)),
    ("binary spread = 3", dict(form="binary", spread=3)),
    ("binary spread < 0", dict(form="binary", spread=-1)),
    ("reserved", dict(reserved=1)),
    ("ld < R", dict(ld=7)),
    ("in place", dict(d_out=1 << 40)),
    ("d_out inside d_in", dict(d_out=(1 << 40) + 4 * 8)),
    ("d_out overlaps d_hist", dict(d_out=(2 << 40) + 4 * 4 * 8)),
    ("binary in place", dict(form="binary", d_out=1 << 40)),
]


@pytest.mark.parametrize("what,kw", BAD, ids=[b[0] for b in BAD])
def test_argument_errors_before_the_context(what, kw):
    capi, lib = _lib()
    rc, msg = _call(lib, capi, **kw)
    assert rc == capi.RSP_ERR_ARG, (what, rc, msg)
    name = "rsp_binint_dev" if kw.get("form") == "binary" else "rsp_integrate_dev"
    assert msg.startswith(name + ":") and "null ctx" not in msg, (what, msg)


@pytest.mark.parametrize("form", ["sum", "binary"])
def test_a_well_formed_call_gets_as_far_as_the_context(form):
    capi, lib = _lib()
    rc, msg = _call(lib, capi, form=form)
    assert rc == capi.RSP_ERR_ARG and "null ctx" in msg
    # n = 1 keeps no planes: d_hist may be NULL
    rc, msg = _call(lib, capi, form=form, n=1, m=0 if form == "sum" else 1, d_hist=None)
    assert rc == capi.RSP_ERR_ARG and "null ctx" in msg


def test_struct_layout_matches_the_header():
    capi, _ = _lib()
    assert C.sizeof(capi.rsp_integ_params) == 32
    assert [f for f, _ in capi.rsp_integ_params._fields_] == ["n", "m", "spread", "reserved", "ld", "cpi_stride"]
    assert capi.rsp_integ_params.ld.offset == 16 and capi.rsp_integ_params.cpi_stride.offset == 24
